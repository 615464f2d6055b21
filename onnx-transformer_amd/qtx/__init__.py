"""qtx — MI355X-native (gfx950) W8A8/W4A8 inference path for the reference's quantized
IWSLT14 transformer (gebegebegebe/onnx-transformer).

Public surface mirrors the reference's entry points:
  InferenceSession(path).run(None, feeds)      ~ onnxruntime.InferenceSession
  run_module(module, feeds, ...)               ~ onnx_optimized_inference.run_module
  greedy_decode(model, src, src_mask, max_len, start_symbol)
  greedy_decode(..., return_scores=True) -> (ys, Scores)   ~ the campaign's torch.topk(prob, 2)
  decode_fault_sweep(model, src, src_mask, max_len, start_symbol, trials)   ~ a campaign's trials
  greedy_decode_kvfault(model, src, src_mask, max_len, fault= | upset=, step=)   a fault of the
                                               KV-cached decode itself (no reference counterpart)
  greedy_decode_kvfault_trials(model, src, src_mask, max_len, start_symbol, trials)   one such
                                               trial per sentence in one decode; kvfault_campaign
  greedy_decode_enctrials(model, src, src_mask, max_len, start_symbol, faults)   one encoder or
                                               memory K/V fault per sentence; encfault_campaign
  score_targets(model, src, src_mask, tgt) -> TargetScores   ~ EncoderDecoder.forward on a given
                                                               target + log_softmax
"""
from .weights import (BOS, DEFAULT_SEED, EOS, PAD, UNK, ModelConfig, load_checkpoint,
                      positional_table, synthetic_state_dict, tensor_order)

__all__ = ["BOS", "EOS", "PAD", "UNK", "DEFAULT_SEED", "ModelConfig", "load_checkpoint",
           "positional_table", "synthetic_state_dict", "tensor_order", "QtxModel",
           "InferenceSession", "run_module", "set_default_model", "greedy_decode",
           "greedy_decode_fault", "greedy_decode_kvfault", "greedy_decode_kvfault_trials",
           "kvfault_campaign", "greedy_decode_enctrials", "encfault_campaign",
           "decode_fault_sweep", "plan_sweep",
           "SweepStats", "Scores", "FaultStepRecord", "make_src_mask", "score_targets",
           "rescore_beam", "TargetScores", "lib"]


def __getattr__(name):
    # lazy: importing qtx must not require a GPU; using the compute entry points does.
    if name in ("QtxModel",):
        from .model import QtxModel
        return QtxModel
    if name in ("InferenceSession", "run_module", "set_default_model"):
        from . import session
        return getattr(session, name)
    if name in ("greedy_decode", "greedy_decode_fault", "greedy_decode_kvfault",
                "greedy_decode_kvfault_trials", "kvfault_campaign", "greedy_decode_enctrials",
                "encfault_campaign",
                "decode_fault_sweep", "plan_sweep", "SweepStats", "Scores", "FaultStepRecord",
                "make_src_mask", "score_targets", "rescore_beam", "TargetScores"):
        from . import decode
        return getattr(decode, name)
    if name == "lib":
        from ._lib import lib
        return lib
    raise AttributeError(name)
