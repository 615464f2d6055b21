"""Host-side handle of the device-resident quantized model.

torch tensors are used only as device containers and for the current HIP stream; every
computation runs in libqtx.so (HIP kernels for gfx950).  If the extension cannot be
loaded, or no GPU is visible, construction raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from .weights import EOS, PAD, ModelConfig, positional_table, tensor_order


def _torch():
    import torch
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device=None):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _on_device(fn):
    """Run a QtxModel entry point with the model's device current: its streams, events
    and workspace then belong to that device whatever device the caller has selected."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with _torch().cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapped


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("qtx needs a ROCm GPU (gfx950); no device is visible")


class QtxModel:
    """Quantized W8A8 (or W4A8) model on one GPU, built from a reference state dict."""

    def __init__(self, state_dict: dict, cfg: ModelConfig = ModelConfig(), device=None):
        torch = _torch()
        require_gpu()
        self.cfg = cfg
        self.device = torch.device(device or "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        self.ccfg = _lib.QtxConfig(cfg.src_vocab, cfg.tgt_vocab, cfg.n_layers, cfg.d_model,
                                   cfg.d_ff, cfg.n_heads, cfg.max_len, cfg.weight_bits)
        keys = tensor_order(cfg)
        n = L.qtx_model_tensor_count(C.byref(self.ccfg))
        if n != len(keys):
            raise RuntimeError(f"tensor count mismatch: lib {n} vs host {len(keys)}")
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(np.ascontiguousarray(state_dict[k], np.float32)
                                    .reshape(-1)).to(self.device) for k in keys]
            pe_np = state_dict.get("src_embed.1.pe")
            pe_np = positional_table(cfg.d_model, cfg.max_len) if pe_np is None else pe_np
            pe = torch.from_numpy(np.ascontiguousarray(pe_np, np.float32).reshape(-1)).to(self.device)
            arr = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
            h = C.c_void_p()
            _lib.call("qtx_model_create", C.byref(self.ccfg), arr, len(dev), _ptr(pe),
                      _stream(self.device), C.byref(h))
        self.handle = h
        self._tls = threading.local()

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _lib.lib().qtx_model_destroy(h)
            except Exception:
                pass
            self.handle = None

    @_on_device
    def check(self):
        """Synchronise the current stream and raise QtxError (status QTX_E_DEVICE) if a
        kernel of this thread's last call on the model flagged an error in the thread's
        device status word (qtx_model_check); called wherever the host synchronises anyway."""
        _lib.call("qtx_model_check", self.handle, _stream(self.device))

    @property
    def device_bytes(self) -> int:
        return int(_lib.lib().qtx_model_device_bytes(self.handle))

    # ---- workspace (grown on demand, reused; never allocated inside a hot call) --------
    # One per calling thread: the handle is shared by threads (include/qtx.h), each with
    # its own stream, so each also needs its own scratch.
    @_on_device
    def workspace(self, nbytes: int):
        torch = _torch()
        ws = getattr(self._tls, "ws", None)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            self._tls.ws = ws
        return ws

    # ---- model-level entry points (device tensors in, device tensors out) -------------
    @_on_device
    def encode(self, x, src_mask_u8, fault=None):
        """x [B,S,512] f32, src_mask_u8 [B,S] uint8 -> memory [B,S,512] f32.
        fault: an optional qtx.fault.Fault (one injected fault, module "Encoder")."""
        torch = _torch()
        B, S, _ = x.shape
        out = torch.empty_like(x)
        nb = _lib.lib().qtx_encoder_workspace_size(self.handle, B, S)
        ws = self.workspace(nb)
        if fault is None:
            _lib.call("qtx_encoder_forward", self.handle, _ptr(x), _ptr(src_mask_u8), B, S,
                      _ptr(out), _ptr(ws), ws.numel(), _stream(self.device))
        else:
            _lib.call("qtx_encoder_forward_fault", self.handle, _ptr(x), _ptr(src_mask_u8), B,
                      S, _ptr(out), _ptr(ws), ws.numel(), C.byref(fault.to_c()), _stream(self.device))
        return out

    @_on_device
    def decode(self, y, memory, src_mask_u8, tgt_mask_u8, fault=None):
        """y [B,T,512], memory [B,S,512], src_mask [B,S] u8, tgt_mask [T,T] or [B,T,T] u8."""
        torch = _torch()
        B, T, _ = y.shape
        S = memory.shape[1]
        out = torch.empty_like(y)
        nb = _lib.lib().qtx_decoder_workspace_size(self.handle, B, T, S)
        ws = self.workspace(nb)
        batched = 1 if tgt_mask_u8.dim() == 3 and tgt_mask_u8.shape[0] == B and B > 1 else 0
        if fault is None:
            _lib.call("qtx_decoder_forward", self.handle, _ptr(y), _ptr(memory),
                      _ptr(src_mask_u8), _ptr(tgt_mask_u8), batched, B, T, S, _ptr(out),
                      _ptr(ws), ws.numel(), _stream(self.device))
        else:
            _lib.call("qtx_decoder_forward_fault", self.handle, _ptr(y), _ptr(memory),
                      _ptr(src_mask_u8), _ptr(tgt_mask_u8), batched, B, T, S, _ptr(out),
                      _ptr(ws), ws.numel(), C.byref(fault.to_c()), _stream(self.device))
        return out

    @_on_device
    def greedy(self, src, src_mask_u8, max_len: int = 72, start: int = 0, out=None, fault=None,
               scores: bool = False):
        """src int64 [B,S], src_mask [B,S] u8 -> ids int64 [B,max_len] (device).
        fault: an optional encoder qtx.fault.Fault.
        scores=True: (ids, top_ids int64 [B,max_len-1,2], top_logp f32 [B,max_len-1,2]), the
        two best tokens of every step and their log-probabilities (qtx_greedy_decode_scored)."""
        torch = _torch()
        B, S = src.shape
        ids = out if out is not None else torch.empty((B, max_len), dtype=torch.int64,
                                                      device=self.device)
        if scores:
            top_ids = torch.empty((B, max_len - 1, 2), dtype=torch.int64, device=self.device)
            top_logp = torch.empty((B, max_len - 1, 2), dtype=torch.float32, device=self.device)
            nb = _lib.lib().qtx_greedy_scored_workspace_size(self.handle, B, S, max_len)
            ws = self.workspace(nb)
            _lib.call("qtx_greedy_decode_scored", self.handle, _ptr(src), _ptr(src_mask_u8), B, S,
                      max_len, int(start), _ptr(ids), _ptr(top_ids), _ptr(top_logp), _ptr(ws),
                      ws.numel(), C.byref(fault.to_c()) if fault is not None else None,
                      _stream(self.device))
            return ids, top_ids, top_logp
        nb = _lib.lib().qtx_greedy_workspace_size(self.handle, B, S, max_len)
        ws = self.workspace(nb)
        if fault is None:
            _lib.call("qtx_greedy_decode", self.handle, _ptr(src), _ptr(src_mask_u8), B, S,
                      max_len, int(start), _ptr(ids), _ptr(ws), ws.numel(), _stream(self.device))
        else:
            _lib.call("qtx_greedy_decode_fault", self.handle, _ptr(src), _ptr(src_mask_u8), B,
                      S, max_len, int(start), _ptr(ids), _ptr(ws), ws.numel(),
                      C.byref(fault.to_c()), _stream(self.device))
        return ids

    @_on_device
    def beam(self, src, src_mask_u8, max_len: int = 72, start: int = 0, beam_size: int = 4,
             eos: int = EOS, pad: int = PAD, early_exit: bool = True):
        """Beam search with EOS stop (qtx_beam_decode).  src int64 [B,S], src_mask [B,S] u8 ->
        (hyp_ids int64 [B,beam,max_len], hyp_score f32 [B,beam], hyp_len int32 [B,beam]) on
        the device, in search order (best raw score first), and steps_run (int): the decoder
        steps launched.  early_exit: stop once every hypothesis has ended (the host reads one
        word back every QTX_GRAPH_STEPS steps); the outputs do not depend on it."""
        torch = _torch()
        B, S = src.shape
        K = int(beam_size)
        hyp_ids = torch.empty((B, max(K, 0), max_len), dtype=torch.int64, device=self.device)
        hyp_score = torch.empty((B, max(K, 0)), dtype=torch.float32, device=self.device)
        hyp_len = torch.empty((B, max(K, 0)), dtype=torch.int32, device=self.device)
        steps = C.c_int32(0)
        nb = _lib.lib().qtx_beam_workspace_size(self.handle, B, S, max_len, K)
        ws = self.workspace(nb)
        _lib.call("qtx_beam_decode", self.handle, _ptr(src), _ptr(src_mask_u8), B, S, max_len, K,
                  int(start), int(eos), int(pad), 1 if early_exit else 0, _ptr(hyp_ids),
                  _ptr(hyp_score), _ptr(hyp_len), C.byref(steps), _ptr(ws), ws.numel(),
                  _stream(self.device))
        return hyp_ids, hyp_score, hyp_len, int(steps.value)

    @_on_device
    def score(self, src, src_mask_u8, tgt, pad: int = PAD, tgt_per_src: int = 1, faults=None,
              return_top2: bool = True):
        """Teacher-forced scoring of given targets (qtx_score_targets).  src int64 [B,S],
        src_mask [B,S] u8, tgt int64 [R,L] with R = B * tgt_per_src (row r a target of sentence
        r // tgt_per_src) -> (tok_logp f32, rank int32 [N+1,R,L-1], top_ids int64, top_logp f32
        [N+1,R,L-1,2] or None, None) on the device: entry t scores tgt[:, t+1] given
        tgt[:, :t+1].  faults: a list of N qtx.fault.Fault (trial 0 is fault-free, trial n
        applies faults[n-1] alone); pad < 0: the causal target mask alone."""
        torch = _torch()
        B, S = src.shape
        R, L = tgt.shape
        K = int(tgt_per_src)
        if K < 1 or R != B * K:
            raise ValueError(f"tgt has {R} rows for {B} sentences x tgt_per_src {K}")
        faults = list(faults or [])
        N = len(faults)
        T = max(L - 1, 0)
        tok_logp = torch.empty((N + 1, R, T), dtype=torch.float32, device=self.device)
        rank = torch.empty((N + 1, R, T), dtype=torch.int32, device=self.device)
        top_ids = top_logp = None
        if return_top2:
            top_ids = torch.empty((N + 1, R, T, 2), dtype=torch.int64, device=self.device)
            top_logp = torch.empty((N + 1, R, T, 2), dtype=torch.float32, device=self.device)
        farr = (_lib.Fault * N)(*[f.to_c() for f in faults]) if N else None
        nb = _lib.lib().qtx_score_workspace_size(self.handle, B, S, L, K, N)
        ws = self.workspace(nb)
        _lib.call("qtx_score_targets", self.handle, _ptr(src), _ptr(src_mask_u8), B, S, _ptr(tgt),
                  L, K, int(pad), farr, N, _ptr(tok_logp), _ptr(rank), _ptr(top_ids),
                  _ptr(top_logp), _ptr(ws), ws.numel(), _stream(self.device))
        return tok_logp, rank, top_ids, top_logp

    @_on_device
    def dfault_workspace(self, B: int, S: int, max_len: int):
        """A workspace of its own for greedy_dfault / greedy_dfault_resume (uint8 device
        tensor): a resume reads what the last call left in it, so it is not the shared
        per-thread scratch of the other entry points."""
        torch = _torch()
        nb = _lib.lib().qtx_greedy_dfault_workspace_size(self.handle, B, S, max_len)
        return torch.empty(max(int(nb), 256), dtype=torch.uint8, device=self.device)

    def _dfault_outputs(self, B, max_len, scores):
        torch = _torch()
        ids = torch.empty((B, max_len), dtype=torch.int64, device=self.device)
        if not scores:
            return ids, None, None, None, None
        top_ids = torch.empty((B, max_len - 1, 2), dtype=torch.int64, device=self.device)
        top_logp = torch.empty((B, max_len - 1, 2), dtype=torch.float32, device=self.device)
        rec_ids = torch.empty((B, 2, 2), dtype=torch.int64, device=self.device)
        rec_logp = torch.empty((B, 2, 2), dtype=torch.float32, device=self.device)
        return ids, top_ids, top_logp, rec_ids, rec_logp

    @_on_device
    def greedy_dfault(self, src, src_mask_u8, fault, fault_step: int, max_len: int = 72,
                      start: int = 0, scores: bool = False, ws=None):
        """KV-cached greedy decode with one decoder fault at step ``fault_step``
        (qtx_greedy_decode_dfault).  src int64 [B,S], src_mask [B,S] u8 -> ids int64
        [B,max_len]; scores=True: (ids, top_ids, top_logp, rec_ids, rec_logp), the record
        [B,2,2] ([:,0] golden, [:,1] faulty top 2) meaningful when fault_step < max_len-1.
        ws: a dfault_workspace to resume on later (default: the thread's scratch)."""
        B, S = src.shape
        ids, top_ids, top_logp, rec_ids, rec_logp = self._dfault_outputs(B, max_len, scores)
        if ws is None:
            ws = self.workspace(_lib.lib().qtx_greedy_dfault_workspace_size(self.handle, B, S, max_len))
        _lib.call("qtx_greedy_decode_dfault", self.handle, _ptr(src), _ptr(src_mask_u8), B, S,
                  max_len, int(start), _ptr(ids), _ptr(top_ids), _ptr(top_logp), _ptr(rec_ids),
                  _ptr(rec_logp), _ptr(ws), ws.numel(),
                  C.byref(fault.to_c()) if fault is not None else None, int(fault_step),
                  _stream(self.device))
        return (ids, top_ids, top_logp, rec_ids, rec_logp) if scores else ids

    @_on_device
    def greedy_dfault_resume(self, ws, B: int, S: int, fault, fault_step: int, max_len: int = 72):
        """One more decoder-fault trial on the workspace a scored greedy_dfault (or a resume)
        left, for the same sentences (qtx_greedy_dfault_resume) -> (ids, top_ids, top_logp,
        rec_ids, rec_logp, changed): changed, a host int32 array [B], says whose token the
        fault changed.  Synchronises the stream."""
        ids, top_ids, top_logp, rec_ids, rec_logp = self._dfault_outputs(B, max_len, True)
        changed = (C.c_int32 * B)()
        _lib.call("qtx_greedy_dfault_resume", self.handle, B, S, max_len, _ptr(ids), _ptr(top_ids),
                  _ptr(top_logp), _ptr(rec_ids), _ptr(rec_logp), _ptr(ws), ws.numel(),
                  C.byref(fault.to_c()) if fault is not None else None, int(fault_step), changed,
                  _stream(self.device))
        return ids, top_ids, top_logp, rec_ids, rec_logp, np.array(changed[:], np.int32)

    @_on_device
    def greedy_kvfault(self, src, src_mask_u8, step: int, fault=None, upset=None,
                       max_len: int = 72, start: int = 0, scores: bool = False):
        """KV-cached greedy decode with one fault of the cached decode itself
        (qtx_greedy_decode_kvfault): ``fault``, a decoder qtx.fault.Fault computed into step
        ``step``'s cached run, or ``upset``, a qtx.fault.CacheUpset flipped in storage before
        step ``step`` — exactly one.  Returns as greedy_dfault: ids, or with scores=True (ids,
        top_ids, top_logp, rec_ids, rec_logp), the record meaningful when step < max_len-1."""
        B, S = src.shape
        ids, top_ids, top_logp, rec_ids, rec_logp = self._dfault_outputs(B, max_len, scores)
        ws = self.workspace(_lib.lib().qtx_greedy_kvfault_workspace_size(self.handle, B, S, max_len))
        _lib.call("qtx_greedy_decode_kvfault", self.handle, _ptr(src), _ptr(src_mask_u8), B, S,
                  max_len, int(start), _ptr(ids), _ptr(top_ids), _ptr(top_logp), _ptr(rec_ids),
                  _ptr(rec_logp), _ptr(ws), ws.numel(),
                  C.byref(fault.to_c()) if fault is not None else None,
                  C.byref(upset.to_c()) if upset is not None else None, int(step),
                  _stream(self.device))
        return (ids, top_ids, top_logp, rec_ids, rec_logp) if scores else ids

    @_on_device
    def greedy_kvtrials(self, src, src_mask_u8, trials, max_len: int = 72, start: int = 0):
        """One KV-cached scored decode with one independent trial per sentence
        (qtx_greedy_decode_kvtrials).  trials: B items, each None or (qtx.fault.Fault |
        qtx.fault.CacheUpset, step) in the coordinates of the B = 1 call on that sentence.
        Returns (ids, top_ids, top_logp, rec_ids, rec_logp) on the device; the record row of a
        sentence whose trial is None or never applied is zeros."""
        from .fault import CacheUpset, Fault
        B, S = src.shape
        if len(trials) != B:
            raise ValueError(f"{len(trials)} trials for {B} sentences")
        arr = (_lib.KvTrial * B)()
        for b, tr in enumerate(trials):
            if tr is None:
                continue
            what, step = tr
            arr[b].step = int(step)
            if isinstance(what, Fault):
                arr[b].what, arr[b].fault = 1, what.to_c()
            elif isinstance(what, CacheUpset):
                arr[b].what, arr[b].upset = 2, what.to_c()
            else:
                raise TypeError(f"trial {b}: a Fault or a CacheUpset, not {type(what).__name__}")
        ids, top_ids, top_logp, rec_ids, rec_logp = self._dfault_outputs(B, max_len, True)
        ws = self.workspace(_lib.lib().qtx_greedy_kvtrials_workspace_size(self.handle, B, S, max_len))
        _lib.call("qtx_greedy_decode_kvtrials", self.handle, _ptr(src), _ptr(src_mask_u8), B, S,
                  max_len, int(start), _ptr(ids), _ptr(top_ids), _ptr(top_logp), _ptr(rec_ids),
                  _ptr(rec_logp), _ptr(ws), ws.numel(), arr, _stream(self.device))
        return ids, top_ids, top_logp, rec_ids, rec_logp

    @_on_device
    def greedy_enctrials(self, src, src_mask_u8, faults, max_len: int = 72, start: int = 0):
        """One scored greedy decode with one encoder-side fault per sentence
        (qtx_greedy_decode_enctrials, include/qtx_enctrials.h).  faults: B items, each None or a
        qtx.fault.Fault — an encoder fault, or a decoder CK / CV fault — in the coordinates of
        the B = 1 call on that sentence.  Returns (ids, top_ids, top_logp) on the device."""
        B, S = src.shape
        if len(faults) != B:
            raise ValueError(f"{len(faults)} faults for {B} sentences")
        arr = (_lib.Fault * B)()
        for b, f in enumerate(faults):
            if f is not None:
                arr[b] = f.to_c()
        ids, top_ids, top_logp, _, _ = self._dfault_outputs(B, max_len, True)
        ws = self.workspace(_lib.lib().qtx_greedy_enctrials_workspace_size(self.handle, B, S, max_len))
        _lib.call("qtx_greedy_decode_enctrials", self.handle, _ptr(src), _ptr(src_mask_u8), B, S,
                  max_len, int(start), _ptr(ids), _ptr(top_ids), _ptr(top_logp), _ptr(ws),
                  ws.numel(), arr, _stream(self.device))
        return ids, top_ids, top_logp

    @_on_device
    def embed(self, ids, which: str = "src", pos0: int = 0):
        torch = _torch()
        B, T = ids.shape
        out = torch.empty((B, T, self.cfg.d_model), dtype=torch.float32, device=self.device)
        _lib.call("qtx_embed", self.handle, 0 if which == "src" else 1, _ptr(ids), B, T, pos0,
                  _ptr(out), _stream(self.device))
        return out

    @_on_device
    def generator(self, x, want_logp: bool = True, return_logits: bool = False):
        """x [M,512] -> (logp [M,V] or None, ids int64 [M]) (+ raw logits [M,V])."""
        torch = _torch()
        M = x.shape[0]
        V = self.cfg.tgt_vocab
        logp = torch.empty((M, V), dtype=torch.float32, device=self.device) if want_logp else None
        ids = torch.empty((M,), dtype=torch.int64, device=self.device)
        ws = torch.empty((M * V,), dtype=torch.float32, device=self.device)
        _lib.call("qtx_generator", self.handle, _ptr(x), M, _ptr(logp), _ptr(ids), _ptr(ws),
                  ws.numel() * 4, _stream(self.device))
        if return_logits:
            return logp, ids, ws.view(M, V)
        return logp, ids

    @_on_device
    def generator_top2(self, x):
        """x [M,512] -> (top_ids int64 [M,2], top_logp f32 [M,2]): torch.topk(prob, 2, dim=1)
        of the generator's log-probabilities (qtx_generator_top2; no [M,V] log-prob write)."""
        torch = _torch()
        M = x.shape[0]
        V = self.cfg.tgt_vocab
        top_ids = torch.empty((M, 2), dtype=torch.int64, device=self.device)
        top_logp = torch.empty((M, 2), dtype=torch.float32, device=self.device)
        ws = torch.empty((M * V,), dtype=torch.float32, device=self.device)
        _lib.call("qtx_generator_top2", self.handle, _ptr(x), M, _ptr(top_ids), _ptr(top_logp),
                  _ptr(ws), ws.numel() * 4, _stream(self.device))
        return top_ids, top_logp


def to_u8_mask(mask, device):
    """Any bool/int mask tensor or array -> contiguous uint8 device tensor (nonzero = keep)."""
    torch = _torch()
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    return (mask != 0).to(torch.uint8).to(device).contiguous()
