"""Generate tests/golden/golden_parity.partNN.npz: the fixtures of the quantitative reference-parity
tests (tests/test_parity_quant.py), from the REFERENCE's own modules.

Run in the build container only (it imports /root/reference, which never travels):

    python tests/golden/make_parity.py

Same model construction as make_golden.py (make_model -> get_quantized -> load_state_dict
with the seeded synthetic weights).  Written (data only, no reference source):

* ``src`` / ``src_mask``: 16 sentences, lengths 8..24 padded to 24 with <blank> = 2.
* ``greedy``: the reference's batched greedy decode (batch_output.py:659-673 semantics:
  71 steps, full-prefix recompute, first-index argmax of the generator's log-probs).
* ``top8`` / ``top8_id``: at every step of that decode, the reference's 8 largest
  log-probs and their token ids (``top8[..., 0] - top8[..., 1]`` is the decision margin).
* ``memory``: the reference encoder output of sentences 0..1.
* ``enc_layers``: the reference encoder's per-layer outputs for sentences 0..1
  (layer input 0 = embedding, then after each of the 6 layers, then the final norm),
  so each layer can be checked teacher-forced (fed the reference's own input).
* ``dec_layers`` / ``dec_ys``: the same for the decoder on those 2 sentences x 16 target
  positions (teacher-forced on the reference's greedy prefix), with the reference memory.
* ``enc_q###`` / ``dec_q###``: every rounding decision the reference takes inside those
  two teacher-forced passes, in call order: the int8 codes
  ``round(x / s)`` of each activation quantizer (quant_linear.py:30-43: W8A8Linear inputs,
  and the Q/K/V output quantizers) and ``round(P * 127)`` of each attention's P
  (attention.py:33-35).  The parity test replays them in the oracle to show that every
  oracle/reference difference is one of these rint decisions at a near-tie.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden import REF, SEED, build_reference_model, import_reference  # noqa: E402


class Recorder:
    """Records the reference's rounding decisions in call order while ``on``: wraps every
    W8A8Linear's act_quant / output_quant (instance attributes, quant_linear.py:75-103)
    and MultiHeadedAttention.attention (the P quantization, attention.py:33-35), without
    changing what they compute."""

    def __init__(self, ref):
        self.ref, self.on, self.calls = ref, False, []

    def attach(self, m):
        import torch
        rec = self
        for mod in m.modules():
            if isinstance(mod, self.ref.ql.W8A8Linear):
                for attr in ("act_quant", "output_quant"):
                    if attr == "output_quant" and mod.output_quant_name == "None":
                        continue
                    orig = getattr(mod, attr)

                    def wrapped(x, _orig=orig):
                        out = _orig(x)
                        if rec.on:
                            s = x.abs().max(dim=-1, keepdim=True)[0].clamp(min=1e-5).div(127)
                            rec.calls.append(torch.round(x.div(s)).to(torch.int8).numpy())
                        return out
                    setattr(mod, attr, wrapped)
        cls = self.ref.attention.MultiHeadedAttention
        orig_attn = cls.attention

        def attention(self_, query, key, value, mask=None, dropout=None):
            out, p = orig_attn(self_, query, key, value, mask=mask, dropout=dropout)
            if rec.on:
                rec.calls.append(torch.round(p * 127).to(torch.int8).numpy())
            return out, p
        cls.attention = attention

    def take(self, nb):
        """The recorded codes of sentences 0..nb-1 (leading batch axis), flattened to the
        oracle's [rows, K] for the quantizers and kept [B, H, Sq, Sk] for P."""
        out = []
        for q in self.calls:
            q = q[:nb]
            out.append(q if q.ndim == 4 else q.reshape(-1, q.shape[-1]))
        self.calls = []
        return out


def main():
    import torch
    torch.set_grad_enabled(False)
    sys.path.insert(0, os.path.join(REPO, "onnx-transformer_amd"))
    from qtx.weights import synthetic_state_dict

    ref = import_reference()
    sd = synthetic_state_dict(SEED, ln_random=True)
    m = build_reference_model(ref, sd)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rng = np.random.default_rng(11)
    B, S, max_len = 16, 24, 72
    src = np.full((B, S), 2, np.int64)
    for b, n in enumerate(rng.integers(8, S + 1, B)):
        src[b, 0] = 0
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
        src[b, n - 1] = 1
    src_mask = (src != 2)[:, None, :]
    memory = m.encode(T(src), T(src_mask))

    ys = torch.zeros((B, 1), dtype=torch.int64)
    top8, top8_id = [], []
    for _ in range(max_len - 1):
        o = m.decode(memory, T(src_mask), ys, ref.utils.subsequent_mask(ys.size(1)).long())
        lp = m.generator(o[:, -1])
        v, i = torch.topk(lp, 8, dim=1)
        _, nxt = torch.max(lp, dim=1)            # the reference's own argmax (first index)
        assert (lp.gather(1, nxt[:, None])[:, 0] == v[:, 0]).all()
        top8.append(v.numpy())
        top8_id.append(i.numpy())
        ys = torch.cat([ys, nxt.unsqueeze(1)], dim=1)

    rec = Recorder(ref)
    rec.attach(m)
    # per-layer encoder outputs (encoder.py:14-18) for sentences 0..3
    nb = nr = 2
    x = m.src_embed(T(src[:nb]))
    enc_layers = [x.numpy()]
    rec.on = True
    for layer in m.encoder.layers:
        x = layer(x, T(src_mask[:nb]))
        enc_layers.append(x.numpy())
    rec.on = False
    enc_layers.append(m.encoder.norm(x).numpy())
    enc_q = rec.take(nr)

    # per-layer decoder outputs (decoder.py:13-16) on the reference's greedy prefix
    Tt = 16
    dys = ys[:nb, :Tt]
    tm = ref.utils.subsequent_mask(Tt).long()
    y = m.tgt_embed(dys)
    dec_layers = [y.numpy()]
    rec.on = True
    for layer in m.decoder.layers:
        y = layer(y, memory[:nb], T(src_mask[:nb]), tm)
        dec_layers.append(y.numpy())
    rec.on = False
    dec_layers.append(m.decoder.norm(y).numpy())
    dec_q = rec.take(nr)

    out = dict(src=src, src_mask=src_mask, memory=memory[:nb].numpy(), greedy=ys.numpy(),
               enc_layers=np.stack(enc_layers), dec_layers=np.stack(dec_layers),
               dec_ys=dys.numpy(), top8=np.stack(top8, 1), top8_id=np.stack(top8_id, 1))
    out.update({f"enc_q{i:03d}": q for i, q in enumerate(enc_q)})
    out.update({f"dec_q{i:03d}": q for i, q in enumerate(dec_q)})
    from golden_io import save_golden
    save_golden("golden_parity", out)
    print({k: v.shape for k, v in out.items()}, "reference:", REF)


if __name__ == "__main__":
    main()
