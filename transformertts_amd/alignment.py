"""Phoneme durations read off the decoder's alignment maps (csrc/alignment.hip, C ABI v20) -- what a trained Transformer-TTS
hands a non-autoregressive student (FastSpeech and its descendants):

    out = extract_durations(alignments, phoneme_lens, mel_lens, method="mas" | "argmax",
                            select="utterance" | "batch" | (layer, head))
    # {'durations': (B, Tp) int64, 'focus_rate': (L, B, H) fp32, 'choice': (B, 2) int64 (layer, head), 'valid': (B,) bool}
    out = teacher_durations(model, phoneme, melspec, phoneme_lens, melspec_lens, **kw)      # ... plus 'pred_melspec'

`alignments` is the list `model(...)['alignments']` or `Synthesizer.synthesize(alignments=True)['alignments']` returns: one
(B, H, Tm, Tp) map per decoder layer.  Every (layer, head) is scored by its focus rate F = mean over the frames t < T_b of
max_n A[t][n]; `select` takes the head with the largest F per utterance, the one with the largest sum over the batch, or a given
one; `method="argmax"` counts, per phoneme, the frames whose largest weight lies on it (FastSpeech), `method="mas"` runs the
monotonic alignment search of Glow-TTS on log A -- durations of at least 1 that sum to the length, `valid[b]` False and a zero
row when T_b < N_b (argmax: `valid` = both lengths positive).  Nothing past the lengths is read.  HIP tensors only; every
decision is made on the device, nothing is read back: the call captures into a HIP graph.
"""
from __future__ import annotations

from ctypes import c_void_p
from typing import Dict, Sequence, Tuple, Union

import torch
from torch import Tensor

METHODS = ("mas", "argmax")
SELECT_MODES = {"utterance": 0, "batch": 1}     # TTTS_ALIGN_SELECT_*; 2 = FIXED
MAX_MAPS = 16                                   # TTTS_ALIGN_MAX_MAPS


def _strides(m: Tensor):
    """(ld_row, ld_head, ld_batch) if the kernels can read `m` (B, H, Tm, Tp) where it lies, else None"""
    B, H, Tm, Tp = m.shape
    if Tp > 1 and m.stride(3) != 1:
        return None
    ld_row = m.stride(2) if Tm > 1 else Tp
    ld_head = m.stride(1) if H > 1 else 0
    ld_batch = m.stride(0) if B > 1 else 0
    if ld_row < Tp or ld_head < 0 or ld_batch < 0:
        return None
    return ld_row, ld_head, ld_batch


def _check(alignments, phoneme_lens, mel_lens, method, select):
    """argument refusals (shapes and names first: they read no data and hold for CPU tensors too) -> (maps, mode, layer, head)"""
    if method not in METHODS:
        raise ValueError(f"extract_durations: method must be one of {METHODS}, got {method!r}")
    maps = list(alignments) if alignments is not None else []
    if not maps:
        raise ValueError("extract_durations: no alignment maps")
    if any(m is None for m in maps):
        raise ValueError("extract_durations: an alignment map is None (the forward ran with need_alignments=False)")
    if len(maps) > MAX_MAPS:
        raise ValueError(f"extract_durations: at most {MAX_MAPS} alignment maps, got {len(maps)}")
    if maps[0].dim() != 4:
        raise ValueError(f"extract_durations: alignment maps are (B, H, Tm, Tp), got {tuple(maps[0].shape)}")
    shape = tuple(maps[0].shape)
    for m in maps:
        if tuple(m.shape) != shape:
            raise ValueError(f"extract_durations: maps differ in shape ({tuple(m.shape)} against {shape})")
    if min(shape) < 1:
        raise ValueError(f"extract_durations: empty alignment maps {shape}")
    B, H = shape[:2]
    for name, lens in (("phoneme_lens", phoneme_lens), ("mel_lens", mel_lens)):
        if tuple(lens.shape) != (B,):
            raise ValueError(f"extract_durations: {name} must have shape ({B},), got {tuple(lens.shape)}")
        if lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"extract_durations: {name} must be integers, got {lens.dtype}")
    if isinstance(select, str):
        if select not in SELECT_MODES:
            raise ValueError(f"extract_durations: select must be 'utterance', 'batch' or (layer, head), got {select!r}")
        mode, layer, head = SELECT_MODES[select], 0, 0
    else:
        try:
            layer, head = (int(i) for i in select)
        except (TypeError, ValueError):
            raise ValueError(f"extract_durations: select must be 'utterance', 'batch' or (layer, head), got {select!r}") from None
        if not (0 <= layer < len(maps) and 0 <= head < H):
            raise ValueError(f"extract_durations: (layer {layer}, head {head}) of {len(maps)} maps with {H} heads")
        mode = 2
    for name, t in [("alignments", m) for m in maps] + [("phoneme_lens", phoneme_lens), ("mel_lens", mel_lens)]:
        if not t.is_cuda:
            raise ValueError(f"extract_durations.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {t.device}")
    for m in maps:
        if m.dtype != torch.float32:
            raise ValueError(f"extract_durations.alignments: expected dtype torch.float32, got {m.dtype}")
    return maps, mode, layer, head


def _operands(maps):
    """the maps as the kernels read them -- in place through their strides where the columns are contiguous, one copy otherwise;
    the search takes ONE set of strides for all maps, so maps that differ in layout are all copied -> (maps, strides)"""
    maps = [m.detach() for m in maps]
    maps = [m if _strides(m) is not None else m.contiguous() for m in maps]
    if len({_strides(m) for m in maps}) > 1:
        maps = [m.contiguous() for m in maps]
    return maps, _strides(maps[0])


def _rowstats(maps, strides, plens, mlens):
    """row statistics of every map -> (argmax (L, B, H, Tm) int32, focus_rate (L, B, H) fp32)"""
    from . import _lib
    from .ops import _p, _stream
    lib = _lib.load()
    B, H, Tm, Tp = maps[0].shape
    L, dev = len(maps), maps[0].device
    argmax = torch.empty(L, B, H, Tm, dtype=torch.int32, device=dev)
    rowmax = torch.empty(B, H, Tm, dtype=torch.float32, device=dev)
    focus = torch.empty(L, B, H, dtype=torch.float32, device=dev)
    for i, m in enumerate(maps):
        _lib.check(lib.ttts_alignment_rowstats(_p(m), *strides, _p(plens), _p(mlens), B, H, Tm, Tp, i, L, _p(argmax), _p(rowmax),
                                               _p(focus), _stream()), "ttts_alignment_rowstats")
    return argmax, focus


def _select(focus, plens, mlens, mode, layer, head):
    """-> (choice (B,) int64 = layer * H + head, pairs (B, 2) int64)"""
    from . import _lib
    from .ops import _p, _stream
    L, B, H = focus.shape
    choice = torch.empty(B, dtype=torch.int64, device=focus.device)
    pairs = torch.empty(B, 2, dtype=torch.int64, device=focus.device)
    _lib.check(_lib.load().ttts_alignment_select(_p(focus), _p(plens), _p(mlens), L, B, H, mode, layer, head, _p(choice), _p(pairs),
                                                 _stream()), "ttts_alignment_select")
    return choice, pairs


def extract_durations(alignments: Sequence[Tensor], phoneme_lens: Tensor, mel_lens: Tensor, method: str = "mas",
                      select: Union[str, Tuple[int, int]] = "utterance") -> Dict[str, Tensor]:
    from . import _lib
    from .ops import _p, _stream
    maps, mode, layer, head = _check(alignments, phoneme_lens, mel_lens, method, select)
    lib = _lib.load()
    plens, mlens = phoneme_lens.to(torch.int64).contiguous(), mel_lens.to(torch.int64).contiguous()
    maps, strides = _operands(maps)
    B, H, Tm, Tp = maps[0].shape
    L, dev = len(maps), maps[0].device
    argmax, focus = _rowstats(maps, strides, plens, mlens)
    choice, pairs = _select(focus, plens, mlens, mode, layer, head)
    dur = torch.empty(B, Tp, dtype=torch.int64, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    if method == "argmax":
        _lib.check(lib.ttts_alignment_durations_argmax(_p(argmax), _p(choice), _p(plens), _p(mlens), L, B, H, Tm, Tp, _p(dur), _p(valid),
                                                       _stream()), "ttts_alignment_durations_argmax")
    else:
        nbytes = lib.ttts_alignment_mas_workspace_bytes(B, Tm, Tp)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        ptrs = (c_void_p * L)(*[m.data_ptr() for m in maps])          # a host array: it travels to the kernel by value
        _lib.check(lib.ttts_alignment_mas(ptrs, L, *strides, _p(choice), _p(plens), _p(mlens), B, H, Tm, Tp, _p(ws), nbytes, _p(dur),
                                          _p(valid), _stream()), "ttts_alignment_mas")
    return {"durations": dur, "focus_rate": focus, "choice": pairs, "valid": valid.view(torch.bool)}


def teacher_durations(model, phoneme: Tensor, melspec: Tensor, phoneme_lens: Tensor, melspec_lens: Tensor, **kw) -> Dict[str, Tensor]:
    """the teacher-forced forward in eval mode under no_grad, then `extract_durations(**kw)` on its maps: the call a FastSpeech
    data-preparation script makes per batch.  -> the dict of `extract_durations` plus 'pred_melspec'.  Every module gets its own
    training flag back (a model with, say, frozen BatchNorm layers left in eval mode stays as it was)."""
    was_training = [(mod, mod.training) for mod in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            out = model(phoneme, melspec, phoneme_lens, melspec_lens, need_alignments=True)
    finally:
        for mod, flag in was_training:
            mod.training = flag
    res = extract_durations(out["alignments"], phoneme_lens, melspec_lens, **kw)
    res["pred_melspec"] = out["pred_melspec"]
    return res
