"""Greedy decoding and the sentence-sharded multi-GPU driver.

``greedy_decode(model, src, src_mask, max_len, start_symbol)`` has the signature and
result of the reference's decode loops (reference/onnx_reference_inference.py:622-646;
batched form batch_output.py:659-673): ``ys`` starts with ``start_symbol`` and grows by
``max_len - 1`` argmax tokens, with no EOS exit.  The whole loop (encoder, cross K/V,
71 KV-cached decoder steps, generator + argmax) runs on the GPU in one library call.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .model import QtxModel, to_u8_mask
from .weights import EOS, PAD


@dataclasses.dataclass
class FaultStepRecord:
    """What the reference's campaign prints at the step it corrupts
    (parallelized_inject_onnx_transformer.py:711-740): torch.topk(prob, 2, dim=1) of the
    generator on the golden decoder output (its ``out_2``: the same prefix, no fault) and on
    the faulty one, and whether the chosen token changed.  Arrays [B, 2] / [B]."""
    step: int
    golden_ids: object
    golden_logp: object
    faulty_ids: object
    faulty_logp: object

    @property
    def token_changed(self):
        return self.golden_ids[..., 0] != self.faulty_ids[..., 0]


@dataclasses.dataclass
class Scores:
    """The two best tokens of every decode step and their log-probabilities: ``top_ids`` int64
    and ``top_logp`` float32 [B, max_len-1, 2] (numpy or torch, like the ids they come with);
    entry t describes the choice of ys[:, t+1], top_ids[..., 0] == ys[:, 1:] (include/qtx.h,
    scored decode).  ``fault_step``: a decoder-fault decode's FaultStepRecord, else None."""
    top_ids: object
    top_logp: object
    fault_step: FaultStepRecord | None = None

    @property
    def margin(self):
        """logp(winner) - logp(runner-up) per step, [B, max_len-1] (>= 0; NaN for a non-finite row)."""
        return self.top_logp[..., 0] - self.top_logp[..., 1]


def greedy_decode(model: QtxModel, src, src_mask, max_len: int, start_symbol: int = 0,
                  return_scores: bool = False):
    """src int64 [B,S] (numpy or torch), src_mask [B,1,S] bool -> ys int64 [B,max_len].
    return_scores=True: (ys, Scores) from the scored KV-cached decode."""
    import torch
    was_numpy = isinstance(src, np.ndarray)
    src_t = torch.from_numpy(np.ascontiguousarray(src)) if was_numpy else src
    B, S = src_t.shape
    srcd = src_t.to(model.device, torch.int64).contiguous()
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    out = model.greedy(srcd, md, max_len=max_len, start=start_symbol, scores=return_scores)
    model.check()
    to_host = (lambda t: t.cpu().numpy()) if was_numpy else (lambda t: t.to(src_t.device))
    if return_scores:
        ys, top_ids, top_logp = out
        return to_host(ys), Scores(to_host(top_ids), to_host(top_logp))
    return to_host(out)


@dataclasses.dataclass
class BeamResult:
    """beam_decode's result (numpy or torch, like the src it came from).  Ranked: ``ids`` int64
    [B, n_best, max_len], ``scores`` float64 [B, n_best] (score / max(len, 1) **
    length_penalty) and ``lengths`` int32 [B, n_best] (tokens after the start symbol, the EOS
    included).  As the library left them, in search order (best raw score first): ``hyp_ids``
    [B, beam, max_len], ``hyp_score`` float32 [B, beam] (cumulative log-probability),
    ``hyp_len`` int32 [B, beam].  ``steps_run``: the decoder steps launched."""
    ids: object
    scores: object
    lengths: object
    hyp_ids: object
    hyp_score: object
    hyp_len: object
    steps_run: int


def rank_hypotheses(hyp_score, hyp_len, length_penalty: float = 0.0):
    """Per sentence the order of the hypotheses by score / max(len, 1) ** length_penalty in
    float64, descending and stable (length_penalty = 0 keeps the library's order).
    hyp_score [B, K], hyp_len [B, K] (numpy) -> (order int64 [B, K], ranked scores float64)."""
    s = np.asarray(hyp_score, np.float64) / np.maximum(np.asarray(hyp_len), 1) ** float(length_penalty)
    order = np.argsort(-s, axis=-1, kind="stable")
    return order, np.take_along_axis(s, order, axis=-1)


def beam_decode(model: QtxModel, src, src_mask, max_len: int, start_symbol: int = 0,
                beam_size: int = 4, eos: int = EOS, pad: int = PAD, length_penalty: float = 0.0,
                n_best: int = 1, early_exit: bool = True) -> BeamResult:
    """Beam search with EOS stop (include/qtx.h, beam search): src int64 [B,S] (numpy or
    torch), src_mask [B,1,S] bool -> BeamResult.  The search itself knows no length
    normalisation; the hypotheses are ranked here (rank_hypotheses) and the n_best first kept."""
    import torch
    if not 1 <= int(n_best) <= int(beam_size):
        raise ValueError(f"n_best {n_best} outside 1 .. beam_size {beam_size}")
    was_numpy = isinstance(src, np.ndarray)
    src_t = torch.from_numpy(np.ascontiguousarray(src)) if was_numpy else src
    B, S = src_t.shape
    srcd = src_t.to(model.device, torch.int64).contiguous()
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    hyp_ids, hyp_score, hyp_len, steps = model.beam(srcd, md, max_len=max_len, start=start_symbol,
                                                    beam_size=beam_size, eos=eos, pad=pad,
                                                    early_exit=early_exit)
    model.check()
    hi, hs, hl = hyp_ids.cpu().numpy(), hyp_score.cpu().numpy(), hyp_len.cpu().numpy()
    order, ranked = rank_hypotheses(hs, hl, length_penalty)
    order, ranked = order[:, :n_best], ranked[:, :n_best]
    ids = np.take_along_axis(hi, order[:, :, None], axis=1)
    lens = np.take_along_axis(hl, order, axis=1)
    out = (ids, ranked, lens, hi, hs, hl)
    if not was_numpy:
        out = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(src_t.device) for a in out)
    return BeamResult(*out, steps_run=steps)


@dataclasses.dataclass
class TargetScores:
    """score_targets' result (numpy or torch, like the src it came from): per target row r and
    position t the model's opinion of the label tgt[r, t+1] given tgt[r, :t+1] (include/qtx.h,
    target scoring).  ``tok_logp`` float32 and ``rank`` int32 [R, T] (rank 0: the label is the
    model's first choice; -1 and NaN for a non-finite row), ``top_ids`` int64 and ``top_logp``
    float32 [R, T, 2] (None without return_top2), ``labels`` int64 [R, T] = tgt[:, 1:].  With
    fault trials every array but ``labels`` has a leading axis of 1 + len(faults), index 0
    golden.  Positions whose label is ``pad`` are computed like any other; ``mask`` excludes
    them (pad < 0: nothing is excluded)."""
    tok_logp: object
    rank: object
    top_ids: object
    top_logp: object
    labels: object
    pad: int = PAD

    @property
    def mask(self):
        """labels != pad, [R, T] bool."""
        return self.labels != self.pad

    @property
    def n_tokens(self):
        """Labels under the mask per row, [R]."""
        return self.mask.sum(-1)

    @property
    def sentence_logp(self):
        """The float64 sum of tok_logp under the mask, [.., R]: correctly rounded (math.fsum),
        so it depends neither on the order of the terms nor on how far the rows are padded."""
        import math
        is_np = isinstance(self.tok_logp, np.ndarray)
        lp = np.asarray(self.tok_logp if is_np else self.tok_logp.cpu().numpy(), np.float64)
        m = np.broadcast_to(np.asarray(self.mask if is_np else self.mask.cpu().numpy()), lp.shape)
        flat = [math.fsum(r[k]) for r, k in zip(lp.reshape(-1, lp.shape[-1]),
                                                m.reshape(-1, lp.shape[-1]))]
        out = np.asarray(flat, np.float64).reshape(lp.shape[:-1])
        if is_np:
            return out
        import torch
        return torch.from_numpy(out).to(self.tok_logp.device)

    @property
    def hits(self):
        """rank == 0 under the mask, [.., R, T] bool: the label is what greedy would pick."""
        return (self.rank == 0) & self.mask


def score_targets(model: QtxModel, src, src_mask, tgt, pad: int = PAD, tgt_per_src: int = 1,
                  faults=None, return_top2: bool = True) -> TargetScores:
    """Teacher-forced scoring (include/qtx.h, target scoring; the reference's
    EncoderDecoder.forward on Batch.tgt / tgt_y, encoder_decoder.py:19-23, batch.py:17-30):
    src int64 [B,S] (numpy or torch), src_mask [B,1,S] bool, tgt int64 [B * tgt_per_src, L]
    (row r a target of sentence r // tgt_per_src) -> TargetScores of the L - 1 labels
    tgt[:, 1:].  One library call: the encoder once on the B sentences, one decoder pass over
    all positions, no [.., V] log-probabilities materialised.  faults: a list of
    qtx.fault.Fault, each a trial of its own on the same call (arrays then [1 + len, R, T],
    index 0 golden; 8-bit weights and tgt_per_src == 1).  A label outside the vocabulary
    raises ValueError."""
    import torch
    was_numpy = isinstance(src, np.ndarray)
    src_t = torch.from_numpy(np.ascontiguousarray(src)) if was_numpy else src
    tgt_t = torch.from_numpy(np.ascontiguousarray(tgt)) if isinstance(tgt, np.ndarray) else tgt
    B, S = src_t.shape
    labels = tgt_t[:, 1:]
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= model.cfg.tgt_vocab):
        raise ValueError(f"a label lies outside the vocabulary [0, {model.cfg.tgt_vocab})")
    srcd = src_t.to(model.device, torch.int64).contiguous()
    tgtd = tgt_t.to(model.device, torch.int64).contiguous()
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    out = model.score(srcd, md, tgtd, pad=pad, tgt_per_src=tgt_per_src, faults=faults,
                      return_top2=return_top2)
    model.check()
    to_host = (lambda t: t.cpu().numpy()) if was_numpy else (lambda t: t.to(src_t.device))
    out = [None if t is None else to_host(t if faults is not None else t[0]) for t in out]
    return TargetScores(*out, labels=to_host(labels.to(torch.int64).contiguous()), pad=int(pad))


def accumulate_logp(tok_logp, lengths):
    """Per row the float32 sequential sum acc = fl32(acc + tok_logp[t]) over t < lengths[r]:
    the accumulation of the beam search's score (include/qtx.h, beam search rule 3)."""
    lp = np.asarray(tok_logp, np.float32)
    n = np.asarray(lengths)
    acc = np.zeros(lp.shape[:-1], np.float32)
    for t in range(lp.shape[-1]):
        acc = np.where(t < n, (acc + lp[..., t]).astype(np.float32), acc)
    return acc


def rescore_beam(model: QtxModel, src, src_mask, beam_result: BeamResult, pad: int = PAD):
    """Score a beam search's own hypotheses teacher-forced (score_targets on ``hyp_ids`` with
    tgt_per_src = beam) and add each one's label log-probabilities up as the search did:
    sequentially in float32 over t < hyp_len.  Returns float32 [B, beam] (numpy), equal to
    ``hyp_score`` bit for bit wherever the scores are finite: the full-prefix pass computes
    the cached steps' log-probabilities exactly."""
    to_np = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    hyp_ids, hyp_len = to_np(beam_result.hyp_ids), to_np(beam_result.hyp_len)
    B, K, L = hyp_ids.shape
    ts = score_targets(model, to_np(src), to_np(src_mask), hyp_ids.reshape(B * K, L), pad=pad,
                       tgt_per_src=K, return_top2=False)
    return accumulate_logp(ts.tok_logp, hyp_len.reshape(B * K)).reshape(B, K)


def greedy_decode_fault(model: QtxModel, src, src_mask, max_len: int, start_symbol: int = 0,
                        fault=None, target_inference_number: int = 1,
                        return_scores: bool = False, kv_cache: bool = False):
    """Greedy decode with one injected fault, the reference campaign's loop
    (parallelized_inject_onnx_transformer.py:536-720): an encoder fault corrupts the single
    encoder run (memory); a decoder fault corrupts only the decoder run of step
    ``target_inference_number - 1`` — every step recomputes the whole prefix, as the
    reference does, so the faulty step changes that step's token and nothing else directly.
    src / src_mask as greedy_decode; returns ys int64 [B, max_len] (numpy).
    return_scores=True: (ys, Scores), numpy.  Encoder fault (or none): the scored KV-cached
    decode.  Decoder fault: every step's top 2 of the faulty decode, and in
    ``Scores.fault_step`` the campaign's record of the corrupted step (:711-740): the top 2
    of one extra fault-free decoder run on the same prefix (the reference's ``out_2``) and of
    the faulty run, and token_changed per sentence.
    kv_cache=True: a decoder fault runs as ONE KV-cached library call
    (qtx_greedy_decode_dfault: cached golden steps up to the corrupted one, one faulty
    full-prefix pass for its token, cached steps after it) with the same results, bit for bit."""
    import torch
    src = np.ascontiguousarray(np.asarray(src), np.int64)
    B, S = src.shape
    dev = model.device
    srcd = torch.from_numpy(src).to(dev)
    md = to_u8_mask(src_mask, dev).reshape(B, S)
    enc_fault = fault if fault is not None and fault.module == 0 else None
    dec_fault = fault if fault is not None and fault.module == 1 else None
    if dec_fault is None:                       # KV-cached fused decode, faulty encoder
        out = model.greedy(srcd, md, max_len=max_len, start=start_symbol, fault=enc_fault,
                           scores=return_scores)
        model.check()
        if return_scores:
            return out[0].cpu().numpy(), Scores(out[1].cpu().numpy(), out[2].cpu().numpy())
        return out.cpu().numpy()
    if kv_cache:
        return _decode_dfault_cached(model, srcd, md, max_len, start_symbol, dec_fault,
                                     target_inference_number, return_scores)
    memory = model.encode(model.embed(srcd, "src"), md)
    model.check()                               # the encode's device errors, before the loop
    ys = torch.full((B, 1), int(start_symbol), dtype=torch.int64, device=dev)
    tops, record = [], None
    for i in range(max_len - 1):
        T = ys.shape[1]
        tm = torch.tril(torch.ones((T, T), dtype=torch.uint8, device=dev))
        faulty = i == target_inference_number - 1
        y = model.embed(ys, "tgt")
        out = model.decode(y, memory, md, tm, fault=dec_fault if faulty else None)
        if not return_scores:
            _, nxt = model.generator(out[:, -1].contiguous(), want_logp=False)
        else:
            top = model.generator_top2(out[:, -1].contiguous())
            tops.append(top)
            nxt = top[0][:, 0]
            if faulty:                          # the golden run of this step (out_2)
                gold = model.generator_top2(model.decode(y, memory, md, tm)[:, -1].contiguous())
                record = FaultStepRecord(i, gold[0].cpu().numpy(), gold[1].cpu().numpy(),
                                         top[0].cpu().numpy(), top[1].cpu().numpy())
        ys = torch.cat([ys, nxt[:, None]], dim=1)
    model.check()
    if not return_scores:
        return ys.cpu().numpy()
    top_ids = torch.stack([t[0] for t in tops], dim=1) if tops else torch.empty((B, 0, 2), dtype=torch.int64)
    top_logp = torch.stack([t[1] for t in tops], dim=1) if tops else torch.empty((B, 0, 2))
    return ys.cpu().numpy(), Scores(top_ids.cpu().numpy(), top_logp.cpu().numpy(), record)


def _fault_step(target_inference_number: int, max_len: int) -> int:
    """The step a campaign's target_inference_number corrupts; max_len - 1 (a step that does
    not exist: the fault is never applied) when the loop never reaches that number."""
    step = int(target_inference_number) - 1
    return step if 0 <= step < max_len - 1 else max_len - 1


def _record(step, rec_ids, rec_logp):
    ri, rl = rec_ids.cpu().numpy(), rec_logp.cpu().numpy()
    return FaultStepRecord(step, ri[:, 0].copy(), rl[:, 0].copy(), ri[:, 1].copy(), rl[:, 1].copy())


def _decode_dfault_cached(model, srcd, md, max_len, start_symbol, fault, target_inference_number,
                          return_scores):
    step = _fault_step(target_inference_number, max_len)
    out = model.greedy_dfault(srcd, md, fault, step, max_len=max_len, start=start_symbol,
                              scores=return_scores)
    model.check()
    if not return_scores:
        return out.cpu().numpy()
    ys, top_ids, top_logp, rec_ids, rec_logp = out
    record = _record(step, rec_ids, rec_logp) if step < max_len - 1 else None
    return ys.cpu().numpy(), Scores(top_ids.cpu().numpy(), top_logp.cpu().numpy(), record)


def greedy_decode_kvfault(model: QtxModel, src, src_mask, max_len: int, start_symbol: int = 0,
                          fault=None, upset=None, step: int = 0, return_scores: bool = False):
    """Greedy decode with one fault of the KV-cached decode itself (qtx_greedy_decode_kvfault;
    the contract is tests/kvfault_ref.py) — what the engine that appends K/V rows and never
    recomputes them does, where greedy_decode_fault follows the campaign's full-prefix loop.
    Exactly one of:
      fault  a decoder qtx.fault.Fault computed into the cached run of step ``step``; its
             coordinates are those of the step's own MatMuls (one row per sentence, self keys
             0 .. step); whatever it leaves in the caches and in ys serves every later step.
             CK / CV: the one-time memory K/V projection, step 0.
      upset  a qtx.fault.CacheUpset: one stored bit of a K/V code or scale flips before step
             ``step`` and stays.
    src / src_mask as greedy_decode; returns ys int64 [B, max_len] (numpy), or with
    return_scores=True (ys, Scores), Scores.fault_step holding the golden and the faulty top 2
    of step ``step`` (None when step >= max_len - 1: nothing runs at or after it)."""
    import torch
    if (fault is None) == (upset is None):
        raise ValueError("greedy_decode_kvfault takes exactly one of fault / upset")
    src = np.ascontiguousarray(np.asarray(src), np.int64)
    B, S = src.shape
    srcd = torch.from_numpy(src).to(model.device)
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    out = model.greedy_kvfault(srcd, md, step, fault=fault, upset=upset, max_len=max_len,
                               start=start_symbol, scores=return_scores)
    model.check()
    if not return_scores:
        return out.cpu().numpy()
    ys, top_ids, top_logp, rec_ids, rec_logp = out
    record = _record(int(step), rec_ids, rec_logp) if 0 <= step < max_len - 1 else None
    return ys.cpu().numpy(), Scores(top_ids.cpu().numpy(), top_logp.cpu().numpy(), record)


def greedy_decode_kvfault_trials(model: QtxModel, src, src_mask, max_len: int,
                                 start_symbol: int = 0, trials=()):
    """One KV-cached scored decode that carries one independent kvfault trial per sentence
    (qtx_greedy_decode_kvtrials; the contract is tests/kvtrials_ref.py): ``trials`` is a list of
    B items, each None (a golden row) or (Fault | CacheUpset, step) in the coordinates of
    greedy_decode_kvfault on that sentence ALONE (linear INPUT / OUTPUT row 0, attention b = 0,
    an upset's row the position within the sentence's cache).  Row b equals that stand-alone
    call bit for bit.  Memory K/V projection faults (CK / CV) are not taken here.
    Returns (ys int64 [B, max_len], Scores, records): records[b] a FaultStepRecord with arrays
    [2] (the golden and the faulty top 2 of row b's own step), or None for a row without an
    applied trial."""
    import torch
    src = np.ascontiguousarray(np.asarray(src), np.int64)
    B, S = src.shape
    trials = list(trials)
    srcd = torch.from_numpy(src).to(model.device)
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    ys, top_ids, top_logp, rec_ids, rec_logp = model.greedy_kvtrials(
        srcd, md, trials, max_len=max_len, start=start_symbol)
    model.check()
    ri, rl = rec_ids.cpu().numpy(), rec_logp.cpu().numpy()
    records = [None if tr is None or not 0 <= int(tr[1]) < max_len - 1 else
               FaultStepRecord(int(tr[1]), ri[b, 0].copy(), rl[b, 0].copy(), ri[b, 1].copy(),
                               rl[b, 1].copy())
               for b, tr in enumerate(trials)]
    return ys.cpu().numpy(), Scores(top_ids.cpu().numpy(), top_logp.cpu().numpy()), records


def kvfault_campaign(model: QtxModel, src_row, mask_row, max_len: int, trials, batch: int = 32,
                     start_symbol: int = 0):
    """A campaign of kvfault trials on ONE sentence: src_row [S] (or [1, S]) and its mask row are
    replicated over ``batch`` rows, ``trials`` (any number of (Fault | CacheUpset, step) or None)
    are cut into batches of ``batch`` — the last padded with None — and each batch is one
    greedy_decode_kvfault_trials call.  Returns one (ys [max_len], Scores with arrays
    [max_len-1, 2], record) per trial, in the caller's order."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    trials = list(trials)
    src = np.repeat(np.asarray(src_row, np.int64).reshape(1, -1), batch, axis=0)
    S = src.shape[1]
    mask = np.repeat((np.asarray(mask_row) != 0).reshape(1, 1, S), batch, axis=0)
    out = []
    for k in range(0, len(trials), batch):
        chunk = trials[k:k + batch]
        ys, sc, recs = greedy_decode_kvfault_trials(
            model, src, mask, max_len, start_symbol, chunk + [None] * (batch - len(chunk)))
        out += [(ys[b].copy(), Scores(sc.top_ids[b].copy(), sc.top_logp[b].copy()), recs[b])
                for b in range(len(chunk))]
    return out


def greedy_decode_enctrials(model: QtxModel, src, src_mask, max_len: int, start_symbol: int = 0,
                            faults=()):
    """One scored greedy decode that carries one independent encoder-side fault per sentence
    (qtx_greedy_decode_enctrials; the contract is tests/enctrials_ref.py): ``faults`` is a list of
    B items, each None (a golden row) or a Fault in the coordinates of the stand-alone call on
    that sentence ALONE — an encoder fault (module 0: Q K V O FFN1 FFN2 QK PV) as
    greedy_decode(.., fault=, return_scores=True) takes it, or a decoder CK / CV fault as
    greedy_decode_kvfault takes it at step 0: linear INPUT / OUTPUT row = the token in [0, S),
    attention b = 0 with Sq = Sk = S.  Row b equals that stand-alone call bit for bit.
    fault.random_fault(.., rows=S) and fault.random_attn_fault(.., B=1, ..) draw in these
    coordinates.  Returns (ys int64 [B, max_len], Scores)."""
    import torch
    src = np.ascontiguousarray(np.asarray(src), np.int64)
    B, S = src.shape
    srcd = torch.from_numpy(src).to(model.device)
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    ys, top_ids, top_logp = model.greedy_enctrials(srcd, md, list(faults), max_len=max_len,
                                                   start=start_symbol)
    model.check()
    return ys.cpu().numpy(), Scores(top_ids.cpu().numpy(), top_logp.cpu().numpy())


def encfault_campaign(model: QtxModel, src_row, mask_row, max_len: int, faults, batch: int = 32,
                      start_symbol: int = 0):
    """A campaign of encoder-side trials on ONE sentence, the twin of kvfault_campaign: src_row
    [S] (or [1, S]) and its mask row are replicated over ``batch`` rows, ``faults`` (any number
    of Fault or None, in greedy_decode_enctrials' coordinates) are cut into batches of ``batch``
    — the last padded with None — and each batch is one greedy_decode_enctrials call.  Returns
    one (ys [max_len], Scores with arrays [max_len-1, 2]) per trial, in the caller's order."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    faults = list(faults)
    src = np.repeat(np.asarray(src_row, np.int64).reshape(1, -1), batch, axis=0)
    S = src.shape[1]
    mask = np.repeat((np.asarray(mask_row) != 0).reshape(1, 1, S), batch, axis=0)
    out = []
    for k in range(0, len(faults), batch):
        chunk = faults[k:k + batch]
        ys, sc = greedy_decode_enctrials(model, src, mask, max_len, start_symbol,
                                         chunk + [None] * (batch - len(chunk)))
        out += [(ys[b].copy(), Scores(sc.top_ids[b].copy(), sc.top_logp[b].copy()))
                for b in range(len(chunk))]
    return out


@dataclasses.dataclass
class SweepStats:
    """decode_fault_sweep's counts: trials in all; ``n_resumed`` whose fault changed a token,
    so the steps after it ran again; ``n_skipped`` whose fault was masked, so nothing ran
    after the faulty pass; ``n_never`` whose step the decode never reaches (golden)."""
    n_trials: int = 0
    n_resumed: int = 0
    n_skipped: int = 0
    n_never: int = 0


def plan_sweep(steps) -> list:
    """The order in which a sweep visits its trials: a permutation of range(len(steps)),
    descending in step and stable for equal steps.  A resumed trial rewrites the KV cache
    above its own step only, so in this order every trial finds its prefix golden."""
    return sorted(range(len(steps)), key=lambda k: -int(steps[k]))


def decode_fault_sweep(model: QtxModel, src, src_mask, max_len: int, start_symbol: int, trials):
    """A campaign's trials on one batch of sentences: ``trials`` = [(Fault, target_inference_number),
    ...], decoder faults only (ValueError otherwise).  One scored golden KV-cached decode, then
    one resume per trial in plan_sweep's order (qtx_greedy_dfault_resume): the faulty pass, and
    the steps after it only when a token changed.  Returns (results, SweepStats): results in the
    caller's order, each (ys, Scores) with Scores.fault_step set, numpy, equal to
    greedy_decode_fault(..., fault, target_inference_number, return_scores=True)."""
    import torch
    trials = list(trials)
    for f, _ in trials:
        if f is None or f.module != 1:
            raise ValueError("decode_fault_sweep takes decoder faults (module 1)")
    stats = SweepStats(n_trials=len(trials))
    if not trials:
        return [], stats
    src = np.ascontiguousarray(np.asarray(src), np.int64)
    B, S = src.shape
    srcd = torch.from_numpy(src).to(model.device)
    md = to_u8_mask(src_mask, model.device).reshape(B, S)
    steps = [_fault_step(tin, max_len) for _, tin in trials]
    ws = model.dfault_workspace(B, S, max_len)
    gold = model.greedy_dfault(srcd, md, trials[0][0], max_len - 1, max_len=max_len,
                               start=start_symbol, scores=True, ws=ws)
    model.check()
    g_ys, g_ids, g_logp = (t.cpu().numpy() for t in gold[:3])
    results = [None] * len(trials)
    for k in plan_sweep(steps):
        if steps[k] >= max_len - 1:
            stats.n_never += 1
            results[k] = (g_ys.copy(), Scores(g_ids.copy(), g_logp.copy(), None))
            continue
        ys, top_ids, top_logp, rec_ids, rec_logp, changed = model.greedy_dfault_resume(
            ws, B, S, trials[k][0], steps[k], max_len=max_len)
        if changed.any():
            stats.n_resumed += 1
        else:
            stats.n_skipped += 1
        results[k] = (ys.cpu().numpy(), Scores(top_ids.cpu().numpy(), top_logp.cpu().numpy(),
                                               _record(steps[k], rec_ids, rec_logp)))
    model.check()
    return results, stats


def make_src_mask(src, pad: int = PAD):
    """Batch.src_mask = (src != pad).unsqueeze(-2)   (batch.py:7)."""
    return (np.asarray(src) != pad)[:, None, :]


def shard_bounds(n: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous, balanced sentence shard of rank (no data-path collective)."""
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def length_sorted_shards(lengths, world: int):
    """SURVEY §8e's partition: sentences sorted by source length (longest first, stable),
    dealt to ranks as contiguous balanced chunks (:func:`shard_bounds`), so every rank
    gets sentences of similar length.  Returns one index array per rank."""
    order = np.argsort(-np.asarray(lengths), kind="stable")
    return [order[slice(*shard_bounds(len(order), world, r))] for r in range(world)]


def gather_ids(dist, ids_local, idx_local, n_global: int, world: int):
    """All-gather every rank's decoded ids (int64 [n_r, L], rows ``idx_local`` of the
    global batch) back into global order on every rank: one padded all_gather of the ids
    and one of the indices (≈0.6 MB for 2048 × 72 ids) after the timed region — not on the
    data path.  Works on gloo (CPU tensors) and nccl/RCCL (device tensors)."""
    import torch
    dev = ids_local.device
    L = ids_local.shape[1]
    n = torch.tensor([ids_local.shape[0]], dtype=torch.int64, device=dev)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    mx = int(max(int(s.item()) for s in sizes))
    buf = torch.full((mx, L), -1, dtype=torch.int64, device=dev)
    buf[:ids_local.shape[0]] = ids_local
    ib = torch.full((mx,), -1, dtype=torch.int64, device=dev)
    ib[:ids_local.shape[0]] = torch.as_tensor(np.asarray(idx_local), dtype=torch.int64, device=dev)
    parts = [torch.empty_like(buf) for _ in range(world)]
    iparts = [torch.empty_like(ib) for _ in range(world)]
    dist.all_gather(parts, buf)
    dist.all_gather(iparts, ib)
    out = np.full((n_global, L), -1, np.int64)
    for p, ip, s in zip(parts, iparts, sizes):
        k = int(s.item())
        out[ip[:k].cpu().numpy()] = p[:k].cpu().numpy()
    return out
