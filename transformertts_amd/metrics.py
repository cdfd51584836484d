"""Free-running synthesis quality (csrc/dtw.hip, C ABI v22): a synthesised mel never has its recording's length, so the two are
compared along the best monotonic warping path -- dynamic time warping (DTW).

    out = dtw_distance(x, x_lens, y, y_lens, metric="l1" | "l2", path=False)
    # {'cost': (B,) fp32, 'path_len': (B,) int64, 'distance': (B,) fp32, 'valid': (B,) bool[, 'path': (B, Tx + Ty - 1, 2) int32]}
    cep = mel_cepstra(mel, n_coef=13, mean=None, std=None)                     # (..., n_mels) -> (..., n_coef)
    res = evaluate_synthesis(synthesizer, phoneme, phoneme_lens, melspec, melspec_lens, max_len=1500, window=None)
    # {'distance', 'cost', 'path_len', 'mel_lens', 'len_ratio', 'unfinished', 'valid'}: per utterance, on the device

x is (B, Tx, C), y is (B, Ty, C), fp32; n_b = x_lens[b], m_b = y_lens[b], clamped to the extents.  Cell cost c[i][j] = sum_k |x[i][k] -
y[j][k]| ("l1") or sqrt(sum_k (x[i][k] - y[j][k])^2) ("l2"); D[0][0] = c[0][0], D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j],
D[i][j-1]); on equal values the diagonal wins, then (i-1, j), then (i, j-1).  `cost` = D[n_b-1][m_b-1], `path_len` the cells of the
backtracked path, `distance` = cost / (path_len * C) for "l1" (the mean absolute difference per mel bin along the path: mel-DTW on
log-mels) and cost / path_len for "l2".  A row with a zero length has `valid` False, zeros and a -1 path.  Nothing past the lengths
is read.  HIP tensors only; every decision is made on the device, nothing is read back: the call captures into a HIP graph.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

METRICS = {"l1": 0, "l2": 1}                    # TTTS_DTW_L1 / TTTS_DTW_L2
MAX_LEN = 4096                                  # frames per side (dtw.hip DTW_MAX_LEN)
MAX_GROUP = 65535                               # utterances one call takes (the grid)
WORKSPACE_CAP = 256 << 20                       # bytes of workspace a call may hold at a time


def _strides(t: Tensor):
    """(ld_row, ld_batch) if the kernels can read `t` (B, T, C) where it lies, else None"""
    B, T, C = t.shape
    if C > 1 and t.stride(2) != 1:
        return None
    ld_row = t.stride(1) if T > 1 else C
    ld_batch = t.stride(0) if B > 1 else 0
    if ld_row < C or ld_batch < 0:
        return None
    return ld_row, ld_batch


def _check(x, x_lens, y, y_lens, metric, workspace_cap):
    """argument refusals (shapes and names first: they read no data and hold for CPU tensors too)"""
    if metric not in METRICS:
        raise ValueError(f"dtw_distance: metric must be one of {tuple(METRICS)}, got {metric!r}")
    if isinstance(workspace_cap, bool) or not isinstance(workspace_cap, int) or workspace_cap < 1:
        raise ValueError(f"dtw_distance: workspace_cap must be a positive number of bytes, got {workspace_cap!r}")
    for name, t in (("x", x), ("y", y)):
        if t.dim() != 3:
            raise ValueError(f"dtw_distance: {name} must be (B, T, C), got {tuple(t.shape)}")
        if min(t.shape) < 1:
            raise ValueError(f"dtw_distance: empty {name} {tuple(t.shape)}")
    if x.size(0) != y.size(0) or x.size(2) != y.size(2):
        raise ValueError(f"dtw_distance: x and y differ in batch or channels ({tuple(x.shape)} against {tuple(y.shape)})")
    B = x.size(0)
    for name, t in (("x", x), ("y", y)):
        if t.size(1) > MAX_LEN:
            raise ValueError(f"dtw_distance: {name} has {t.size(1)} frames, above the {MAX_LEN} the kernels take")
    for name, lens in (("x_lens", x_lens), ("y_lens", y_lens)):
        if tuple(lens.shape) != (B,):
            raise ValueError(f"dtw_distance: {name} must have shape ({B},), got {tuple(lens.shape)}")
        if lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"dtw_distance: {name} must be integers, got {lens.dtype}")
    for name, t in (("x", x), ("x_lens", x_lens), ("y", y), ("y_lens", y_lens)):
        if not t.is_cuda:
            raise ValueError(f"dtw_distance.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {t.device}")
    for name, t in (("x", x), ("y", y)):
        if t.dtype != torch.float32:
            raise ValueError(f"dtw_distance.{name}: expected dtype torch.float32, got {t.dtype}")


def group_size(B: int, Tx: int, Ty: int, workspace_cap: int = WORKSPACE_CAP) -> int:
    """utterances `dtw_distance` hands the kernels at a time: as many as keep the workspace under `workspace_cap` bytes, one at
    the least (a single utterance at the largest lengths needs about 70 MB)"""
    from . import _lib
    per = _lib.load().ttts_dtw_workspace_bytes(1, Tx, Ty)
    return max(1, min(B, MAX_GROUP, workspace_cap // per))


def _dtw_into(x, x_lens, y, y_lens, metric: int, ws, cost, path_len, distance, valid, path=None) -> None:
    """one ttts_dtw call on operands as the kernels read them, into the caller's arrays"""
    from . import _lib
    from .ops import _p, _stream
    B, Tx, C = x.shape
    (ldx_row, ldx_batch), (ldy_row, ldy_batch) = _strides(x), _strides(y)
    _lib.check(_lib.load().ttts_dtw(_p(x), ldx_row, ldx_batch, _p(x_lens), _p(y), ldy_row, ldy_batch, _p(y_lens), B, Tx, y.size(1), C,
                                    metric, _p(ws), ws.numel() * ws.element_size(), _p(cost), _p(path_len), _p(distance), _p(valid),
                                    _p(path), _stream()), "ttts_dtw")


def dtw_distance(x: Tensor, x_lens: Tensor, y: Tensor, y_lens: Tensor, metric: str = "l1", path: bool = False,
                 workspace_cap: int = WORKSPACE_CAP) -> Dict[str, Tensor]:
    from . import _lib
    _check(x, x_lens, y, y_lens, metric, workspace_cap)
    x, y = x.detach(), y.detach()
    x = x if _strides(x) is not None else x.contiguous()
    y = y if _strides(y) is not None else y.contiguous()
    xl, yl = x_lens.to(torch.int64).contiguous(), y_lens.to(torch.int64).contiguous()
    B, Tx, _ = x.shape
    Ty, dev = y.size(1), x.device
    cost = torch.empty(B, dtype=torch.float32, device=dev)
    dist = torch.empty(B, dtype=torch.float32, device=dev)
    plen = torch.empty(B, dtype=torch.int64, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    cells = torch.empty(B, Tx + Ty - 1, 2, dtype=torch.int32, device=dev) if path else None
    G = group_size(B, Tx, Ty, workspace_cap)
    ws = torch.empty(_lib.load().ttts_dtw_workspace_bytes(G, Tx, Ty) // 4, dtype=torch.float32, device=dev)
    for b0 in range(0, B, G):                   # the groups share the workspace: they run one after the other on the stream
        s = slice(b0, min(B, b0 + G))
        _dtw_into(x[s], xl[s], y[s], yl[s], METRICS[metric], ws, cost[s], plen[s], dist[s], valid[s], cells[s] if path else None)
    out = {"cost": cost, "path_len": plen, "distance": dist, "valid": valid.view(torch.bool)}
    if path:
        out["path"] = cells
    return out


_dct_cache: dict = {}


def dct_basis(n_mels: int, n_coef: int, device=None, dtype=torch.float32) -> Tensor:
    """rows 1 .. n_coef of the orthonormal DCT-II matrix over `n_mels` points, (n_coef, n_mels): basis[c-1][k] =
    sqrt(2 / n_mels) cos(pi (k + 1/2) c / n_mels), built in fp64"""
    k = torch.arange(n_mels, dtype=torch.float64)
    c = torch.arange(1, n_coef + 1, dtype=torch.float64)
    basis = math.sqrt(2.0 / n_mels) * torch.cos(math.pi / n_mels * (k[None, :] + 0.5) * c[:, None])
    return basis.to(device=device, dtype=dtype)


def mel_cepstra(mel: Tensor, n_coef: int = 13, mean: Optional[Tensor] = None, std: Optional[Tensor] = None) -> Tensor:
    """mel-cepstral coefficients 1 .. n_coef of log-mel frames (..., n_mels): the orthonormal DCT-II over the mel axis without its
    coefficient 0 (the frame's energy), one GEMM against a constant basis.  `mean` / `std`: the statistics a normalised mel is
    taken back to the log-mel with first, mel * (std + 1e-8) + mean (the inverse of the data set's normalisation).
    `dtw_distance(mel_cepstra(a), a_lens, mel_cepstra(b), b_lens, metric="l2")['distance'] * 10 * sqrt(2) / ln 10` is MCD-DTW."""
    n_mels = mel.size(-1)
    if isinstance(n_coef, bool) or not isinstance(n_coef, int) or not 1 <= n_coef < n_mels:
        raise ValueError(f"mel_cepstra: n_coef must be an integer in [1, n_mels = {n_mels}), got {n_coef!r}")
    if (mean is None) != (std is None):
        raise ValueError("mel_cepstra: give both `mean` and `std`, or neither")
    if not mel.is_cuda:
        raise ValueError(f"mel_cepstra.mel: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {mel.device}")
    if mel.dtype != torch.float32:
        raise ValueError(f"mel_cepstra.mel: expected dtype torch.float32, got {mel.dtype}")
    from . import ops
    key = (n_mels, n_coef, mel.device)
    basis = _dct_cache.get(key)
    if basis is None:
        basis = _dct_cache[key] = dct_basis(n_mels, n_coef, mel.device)
    mel = mel.detach()
    if mean is not None:
        mel = mel * (std + 1e-8) + mean
    with torch.no_grad():
        return ops.linear(mel.contiguous(), basis)


def evaluate_synthesis(synthesizer, phoneme: Tensor, phoneme_lens: Tensor, melspec: Tensor, melspec_lens: Tensor, max_len: int = 1500,
                       stop_threshold: float = 0.5, window=None, metric: str = "l1", which: str = "post_melspec") -> Dict[str, Tensor]:
    """`synthesizer.synthesize(phoneme, phoneme_lens, ...)`, then the DTW of what it made (`which`: 'post_melspec' or
    'pred_melspec') against the recording `melspec` (B, T, n_mels) of lengths `melspec_lens`.  -> per utterance, on the device:
    `distance`, `cost`, `path_len`, `valid` of `dtw_distance`, the synthesised `mel_lens`, `len_ratio` = mel_lens / melspec_lens
    (fp32, 0 where melspec_lens is 0) and `unfinished` (bool): the row ran into `max_len` - 1 frames without a stop.  No host read
    beyond what `synthesize` makes per chunk of frames."""
    if which not in ("post_melspec", "pred_melspec"):
        raise ValueError(f"evaluate_synthesis: which must be 'post_melspec' or 'pred_melspec', got {which!r}")
    if metric not in METRICS:
        raise ValueError(f"evaluate_synthesis: metric must be one of {tuple(METRICS)}, got {metric!r}")
    if melspec.dim() != 3:
        raise ValueError(f"evaluate_synthesis: melspec must be (B, T, n_mels), got {tuple(melspec.shape)}")
    if phoneme.dim() != 2 or phoneme.size(0) != melspec.size(0):
        raise ValueError(f"evaluate_synthesis: phoneme must be (B, Tp) = ({melspec.size(0)}, Tp), got {tuple(phoneme.shape)}")
    if tuple(melspec_lens.shape) != (melspec.size(0),):
        raise ValueError(f"evaluate_synthesis: melspec_lens must have shape ({melspec.size(0)},), got {tuple(melspec_lens.shape)}")
    if melspec_lens.dtype.is_floating_point or melspec_lens.dtype == torch.bool:
        raise ValueError(f"evaluate_synthesis: melspec_lens must be integers, got {melspec_lens.dtype}")
    out = synthesizer.synthesize(phoneme, phoneme_lens, max_len=max_len, stop_threshold=stop_threshold, window=window)
    mel_lens = out["mel_lens"]
    res = dtw_distance(out[which], mel_lens, melspec, melspec_lens, metric=metric)
    ref = melspec_lens.to(mel_lens.device)
    ratio = mel_lens.to(torch.float32) / ref.clamp(min=1).to(torch.float32)
    return {"distance": res["distance"], "cost": res["cost"], "path_len": res["path_len"], "valid": res["valid"], "mel_lens": mel_lens,
            "len_ratio": torch.where(ref > 0, ratio, torch.zeros_like(ratio)), "unfinished": mel_lens == int(max_len) - 1}
