"""FastSpeech 2's variance predictor on the kernels of csrc/predictor.hip: `ragged_conv_norm`, a length-masked
Conv1d -> ReLU -> LayerNorm -> Dropout stage in one launch (an implicit GEMM on the fp32-input MFMA with the normalisation as
its epilogue), `RaggedConvNorm`, the stage as a module, and `KernelVariancePredictor`, two stages and the `ttts_rowdot` head: what
`variance.VariancePredictor` computes in stock torch, with the same `state_dict`.  Nothing at or behind a length is read, no
utterance's result depends on another row of the batch, every sum has a fixed order (the same bits on every call), nothing is
read back to the host, and there is no CPU fallback."""
from __future__ import annotations

import math

import torch
from torch import nn

from .variance import _lens

MAX_PHONEMES = 4096          # RC_MAX_P of csrc/predictor.hip
MAX_CIN = 1024               # RC_MAX_CIN
MAX_COUT = 256               # RC_COLS: a workgroup owns a whole output row
MAX_TAPS = 9                 # RC_MAX_TAPS

__all__ = ["ragged_conv_norm", "RaggedConvNorm", "KernelVariancePredictor"]


# ------------------------------------------------------------------------------------------------ checks
def _rows(x, fn):
    """(B, Pmax, Cin) fp32 on the device, handed on through its strides when they allow float4 rows -> x, ld_row, ld_batch"""
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{fn}: x must be (B, Pmax, Cin), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise ValueError(f"{fn}.x: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {x.device}")
    if x.dtype != torch.float32:
        raise ValueError(f"{fn}.x: expected dtype {torch.float32}, got {x.dtype}")
    B, Pmax, C = x.shape
    if C % 4 != 0 or not 4 <= C <= MAX_CIN:
        raise ValueError(f"{fn}: Cin must be a multiple of 4 in [4, {MAX_CIN}], got {C}")
    if Pmax > MAX_PHONEMES:
        raise ValueError(f"{fn}: Pmax must be in [1, {MAX_PHONEMES}] phonemes, got {Pmax}")
    if B > 65535:
        raise ValueError(f"{fn}: B must be in [1, 65535], got {B}")
    ok = x.stride(2) == 1 and x.data_ptr() % 16 == 0
    ok = ok and (Pmax == 1 or (x.stride(1) >= C and x.stride(1) % 4 == 0))
    ld_row = x.stride(1) if Pmax > 1 else C
    ok = ok and (B == 1 or (x.stride(0) % 4 == 0 and x.stride(0) >= (Pmax - 1) * ld_row + C))
    if not ok:
        x = x.contiguous()
        ld_row = C
    return x, ld_row, (x.stride(0) if B > 1 else Pmax * ld_row)


def _param(t, shape, fn, name):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{fn}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{fn}.{name}: expected a {torch.float32} CUDA/HIP tensor, got {t.dtype} on {t.device}")
    return t.contiguous()


def _drop(p, fn):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{fn}: drop_p must be in [0, 1), got {p}")
    return p


# ------------------------------------------------------------------------------------------------ the stage
class _RaggedConvNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ld_row, ld_batch, lens, weight, bias, gamma, beta, eps, drop_p, seed):
        from . import _lib
        from .ops import _p, _ss, _stream
        B, Pmax, Cin = x.shape
        Cout, _, taps = weight.shape
        dev = x.device
        grads = any(ctx.needs_input_grad)
        y = torch.empty(B, Pmax, Cout, dtype=torch.float32, device=dev)
        r = torch.empty(B, Pmax, Cout, dtype=torch.float32, device=dev) if grads else None
        mean = torch.empty(B, Pmax, dtype=torch.float32, device=dev) if grads else None
        rstd = torch.empty(B, Pmax, dtype=torch.float32, device=dev) if grads else None
        xm = torch.empty(B, Pmax, Cin, dtype=torch.float32, device=dev) if ctx.needs_input_grad[4] else None
        ss = _ss()
        _lib.check(_lib.load().ttts_ragged_conv_norm_fwd(_p(x), ld_row, ld_batch, _p(lens), _p(weight), _p(bias), _p(gamma), _p(beta), B,
                                                         Pmax, Cin, Cout, taps, eps, drop_p, seed, ss, _p(y), _p(r), _p(mean), _p(rstd),
                                                         _p(xm), _stream()), "ttts_ragged_conv_norm_fwd")
        ctx.save_for_backward(r, mean, rstd, xm, lens, weight, gamma)
        ctx.shape = (B, Pmax, Cin, Cout, taps)
        ctx.drop = (drop_p, seed, ss)      # backward regenerates the dropout mask under the step-state word of ITS forward
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import _lib
        from .ops import _p, _stream, _ws
        lib = _lib.load()
        r, mean, rstd, xm, lens, weight, gamma = ctx.saved_tensors
        B, Pmax, Cin, Cout, taps = ctx.shape
        drop_p, seed, ss = ctx.drop
        dev = dy.device
        dy = dy.contiguous()
        dx = torch.empty(B, Pmax, Cin, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight) if xm is not None else None
        dbias, dgamma, dbeta = (torch.empty(Cout, dtype=torch.float32, device=dev) for _ in range(3))
        ws = _ws(lib.ttts_ragged_conv_norm_workspace_bytes(B, Pmax, Cin, Cout, taps), dev)
        _lib.check(lib.ttts_ragged_conv_norm_bwd(_p(dy), _p(r), _p(mean), _p(rstd), _p(xm), _p(lens), _p(weight), _p(gamma), B, Pmax, Cin,
                                                 Cout, taps, drop_p, seed, ss, _p(dx), _p(dw), _p(dbias), _p(dgamma), _p(dbeta), _p(ws),
                                                 ws.numel() * 4, 0, _stream()), "ttts_ragged_conv_norm_bwd")
        need = ctx.needs_input_grad
        return (dx, None, None, None, dw, dbias if need[5] else None, dgamma if need[6] else None, dbeta if need[7] else None,
                None, None, None)


def ragged_conv_norm(x, lens, weight, bias, gamma, beta, eps=1e-5, drop_p=0.0, seed=0, training=True):
    """Dropout(LayerNorm(ReLU(Conv1d(x)))) over the phonemes of ragged utterances, one launch (csrc/predictor.hip).  x (B, Pmax,
    Cin) fp32, a strided view goes through its strides; lens (B,) integers; weight (Cout, Cin, k) and bias (Cout,) as `nn.Conv1d`
    holds them (k odd, padding k // 2); gamma, beta (Cout,) as `nn.LayerNorm` -> (B, Pmax, Cout).  Rows at or behind lens[b]
    count as zeros for the taps (their memory is not read: a NaN there does not leak) and are exact zeros in the result and in
    the gradient of x.  drop_p > 0 with training=True drops elements by the counter-based hash of the flat output index under
    `seed` (`ops.seeds.next()` per call, as every dropout site of `ops`) and the active step state; training=False ignores drop_p.
    Cin a multiple of 4 up to 1024, Cout a multiple of 32 up to 256, k odd up to 9."""
    fn = "ragged_conv_norm"
    x, ld_row, ld_batch = _rows(x, fn)
    B, Pmax, Cin = x.shape
    lens = _lens(lens, B, fn, "lens", x.device)
    if weight.dim() != 3 or weight.size(1) != Cin:
        raise ValueError(f"{fn}: weight must be (Cout, {Cin}, k), got {tuple(weight.shape)}")
    Cout, _, taps = weight.shape
    if Cout % 32 != 0 or not 32 <= Cout <= MAX_COUT:
        raise ValueError(f"{fn}: Cout must be a multiple of 32 in [32, {MAX_COUT}], got {Cout}")
    if taps % 2 == 0 or not 1 <= taps <= MAX_TAPS:
        raise ValueError(f"{fn}: the kernel size must be odd in [1, {MAX_TAPS}], got {taps}")
    weight = _param(weight, (Cout, Cin, taps), fn, "weight")
    bias, gamma, beta = (_param(t, (Cout,), fn, name) for t, name in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")))
    eps = float(eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"{fn}: eps must be positive and finite, got {eps}")
    drop_p = _drop(drop_p, fn) if training else 0.0
    return _RaggedConvNorm.apply(x, ld_row, ld_batch, lens, weight, bias, gamma, beta, eps, drop_p, int(seed) & 0xFFFFFFFFFFFFFFFF)


class RaggedConvNorm(nn.Module):
    """`ragged_conv_norm` as a module: `conv` (an `nn.Conv1d` that holds the weights; its own forward is not used) and `norm` (an
    `nn.LayerNorm`), so the parameters carry their names and shapes.  (x (B, Pmax, cin), lens) -> (B, Pmax, cout)."""

    def __init__(self, cin, cout, kernel_size=3, dropout=0.0):
        super().__init__()
        if kernel_size < 1 or kernel_size % 2 == 0 or kernel_size > MAX_TAPS:
            raise ValueError(f"RaggedConvNorm: kernel_size must be odd in [1, {MAX_TAPS}], got {kernel_size}")
        self.conv = nn.Conv1d(cin, cout, kernel_size, padding=kernel_size // 2)
        self.norm = nn.LayerNorm(cout)
        self.dropout = _drop(dropout, "RaggedConvNorm")

    def forward(self, x, lens):
        from . import ops
        p = self.dropout if self.training else 0.0
        return ragged_conv_norm(x, lens, self.conv.weight, self.conv.bias, self.norm.weight, self.norm.bias, eps=self.norm.eps,
                                drop_p=p, seed=ops.seeds.next() if p > 0 else 0)


# ------------------------------------------------------------------------------------------------ the head, the predictor
class _MaskedRowDot(torch.autograd.Function):
    """out[b, p] = h[b, p, :] . w + bias for p < lens[b], exact 0 behind it: ttts_rowdot_fwd / _bwd and ttts_mask_rows.  h is a
    stage's output: zeros behind the lengths."""

    @staticmethod
    def forward(ctx, h, lens, w, bias):
        from . import _lib
        from .ops import _p, _stream
        lib = _lib.load()
        B, Pmax, d = h.shape
        out = torch.empty(B, Pmax, dtype=torch.float32, device=h.device)
        _lib.check(lib.ttts_rowdot_fwd(_p(h), _p(w), _p(bias), _p(out), B * Pmax, d, _stream()), "ttts_rowdot_fwd")
        _lib.check(lib.ttts_mask_rows(_p(out), _p(lens), B, 1, Pmax, 1, _stream()), "ttts_mask_rows")
        ctx.save_for_backward(h, lens, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import _lib
        from .ops import _p, _stream, _ws
        lib = _lib.load()
        h, lens, w = ctx.saved_tensors
        B, Pmax, d = h.shape
        g = dout.clone(memory_format=torch.contiguous_format)      # (a copy: whatever stands behind a length is overwritten, not used)
        _lib.check(lib.ttts_mask_rows(_p(g), _p(lens), B, 1, Pmax, 1, _stream()), "ttts_mask_rows")
        dh = torch.empty_like(h)
        _lib.check(lib.ttts_zero(_p(dh), dh.numel() * 4, _stream()), "ttts_zero")
        dw, db = torch.empty_like(w), torch.empty(1, dtype=torch.float32, device=h.device)
        ws = _ws(lib.ttts_rowdot_bwd_workspace_bytes(d), h.device)
        _lib.check(lib.ttts_rowdot_bwd(_p(g), _p(h), _p(w), _p(dh), _p(dw), _p(db), _p(ws), ws.numel() * 4, B * Pmax, d, 0, None,
                                       _stream()), "ttts_rowdot_bwd")
        return dh, None, dw, db


class KernelVariancePredictor(nn.Module):
    """`VariancePredictor` on the library's kernels: two `ragged_conv_norm` stages and the row-dot head, zero behind the lengths.
    (x (B, Pmax, d_model), phoneme_lens) -> (B, Pmax).  The parameters are those of `VariancePredictor`, name for name and shape
    for shape (conv1, norm1, conv2, norm2, out), so a checkpoint of either loads into the other with strict=True, and
    `VarianceAdaptor(d_model, predictor=KernelVariancePredictor)` takes it.  hidden: a multiple of 32 up to 256."""

    def __init__(self, d_model, hidden=256, kernel_size=3, dropout=0.5):
        super().__init__()
        if kernel_size < 1 or kernel_size % 2 == 0 or kernel_size > MAX_TAPS:
            raise ValueError(f"KernelVariancePredictor: kernel_size must be odd in [1, {MAX_TAPS}], got {kernel_size}")
        if hidden % 32 != 0 or not 32 <= hidden <= MAX_COUT:
            raise ValueError(f"KernelVariancePredictor: hidden must be a multiple of 32 in [32, {MAX_COUT}], got {hidden}")
        if d_model % 4 != 0 or not 4 <= d_model <= MAX_CIN:
            raise ValueError(f"KernelVariancePredictor: d_model must be a multiple of 4 in [4, {MAX_CIN}], got {d_model}")
        pad = kernel_size // 2
        self.conv1, self.conv2 = nn.Conv1d(d_model, hidden, kernel_size, padding=pad), nn.Conv1d(hidden, hidden, kernel_size, padding=pad)
        self.norm1, self.norm2 = nn.LayerNorm(hidden), nn.LayerNorm(hidden)
        self.dropout = _drop(dropout, "KernelVariancePredictor")
        self.out = nn.Linear(hidden, 1)

    def forward(self, x, phoneme_lens):
        from . import ops
        p = self.dropout if self.training else 0.0
        h = x
        for conv, norm in ((self.conv1, self.norm1), (self.conv2, self.norm2)):
            h = ragged_conv_norm(h, phoneme_lens, conv.weight, conv.bias, norm.weight, norm.bias, eps=norm.eps, drop_p=p,
                                 seed=ops.seeds.next() if p > 0 else 0)
        lens = _lens(phoneme_lens, h.size(0), "KernelVariancePredictor", "phoneme_lens", h.device)
        return _MaskedRowDot.apply(h, lens, self.out.weight, self.out.bias)
