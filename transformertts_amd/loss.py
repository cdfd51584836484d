"""TransformerTTSLoss -- masked MSE (pred + 0.5 * post) + stop-gate BCE-with-logits (pos_weight).

Same constructor, call signature, returned dict and `pos_weight` buffer as the reference's `loss.py:8-55`.
The whole loss (and its backward) runs in the fused kernels of csrc/loss.hip: one
streaming masked reduction instead of the reference's boolean-index gathers (`mel[mask]`, loss.py:34-36,44), which
allocate data-dependent shapes and force a device->host sync.  HIP tensors only.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor


class TransformerTTSLoss(nn.Module):
    def __init__(self, stop_weight: float = 8.0):
        super().__init__()
        self.register_buffer("pos_weight", torch.tensor(stop_weight))
        self._pos_weight_host = float(stop_weight)   # host copy: reading the device buffer every step would synchronise

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + "pos_weight" in state_dict:
            self._pos_weight_host = float(state_dict[prefix + "pos_weight"])

    def forward(self, outputs: Dict[str, Tensor], mel: Tensor, lengths: Tensor) -> Dict[str, Tensor]:
        from . import ops          # rejects non-HIP tensors: there is no CPU path (the CPU restatement is oracle/)
        pred, post, stop = outputs["pred_melspec"], outputs["post_melspec"], outputs["pred_stop"]
        total, pred_mel, post_mel, stop_l = ops.TTSLossFn.apply(pred, post, stop, mel, lengths.to(torch.int64),
                                                                self._pos_weight_host)
        return {"total": total, "pred_mel": pred_mel, "post_mel": post_mel, "stop": stop_l}


class GuidedAttentionLoss(nn.Module):
    """Guided attention loss of Transformer-TTS recipes on `output['alignments']` (no counterpart in the reference, which only
    plots its alignments): with W_b[t, n] = 1 - exp(-(n / N_b - t / T_b)^2 / (2 sigma^2)) inside the utterance's (T_b, N_b)
    rectangle and 0 outside, the mean of A o W over the valid positions of the selected heads of the selected decoder layers.
    `heads` / `layers`: None = all, else the indices that count.  It trains the model only on maps that carry a gradient:
    `TransformerTTS.forward(..., alignments_grad=True)`; the default maps are detached.  HIP tensors only (csrc/guided.hip)."""

    def __init__(self, sigma: float = 0.4, heads: Optional[Sequence[int]] = None, layers: Optional[Sequence[int]] = None):
        super().__init__()
        if not sigma > 0:
            raise ValueError(f"GuidedAttentionLoss: sigma {sigma} must be positive")
        for name, sel in (("heads", heads), ("layers", layers)):
            if sel is not None:
                sel = list(sel)
                if not sel:
                    raise ValueError(f"GuidedAttentionLoss: `{name}` selects nothing")
                if any(int(i) != i or i < 0 for i in sel) or len(set(sel)) != len(sel):
                    raise ValueError(f"GuidedAttentionLoss: `{name}` must be distinct non-negative indices, got {sel}")
        self.sigma = float(sigma)
        self.heads = None if heads is None else sorted(int(i) for i in heads)
        self.layers = None if layers is None else sorted(int(i) for i in layers)

    def forward(self, alignments: Sequence[Tensor], phoneme_lens: Tensor, melspec_lens: Tensor) -> Tensor:
        from . import ops
        maps = list(alignments)
        if self.layers is not None:
            if self.layers[-1] >= len(maps):
                raise ValueError(f"GuidedAttentionLoss: layer {self.layers[-1]} of {len(maps)} alignment maps")
            maps = [maps[i] for i in self.layers]
        if not maps or any(m is None for m in maps):
            raise ValueError("GuidedAttentionLoss: no alignment maps (the forward ran with need_alignments=False)")
        head_mask = 0
        if self.heads is not None:
            H = maps[0].shape[1]
            if self.heads[-1] >= H:
                raise ValueError(f"GuidedAttentionLoss: head {self.heads[-1]} of {H} heads")
            if H > 64:
                raise ValueError(f"GuidedAttentionLoss: a head selection takes at most 64 heads, the maps have {H}")
            for h in self.heads:
                head_mask |= 1 << h
        return ops.GuidedAttentionFn.apply(phoneme_lens.to(torch.int64), melspec_lens.to(torch.int64), self.sigma, head_mask, *maps)
