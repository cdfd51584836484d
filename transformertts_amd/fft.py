"""The body of a FastSpeech-2 student on the library's kernels: `ragged_conv_ffn`, the conv feed-forward sublayer
of an FFT block (Conv1d -> ReLU -> Conv1d -> Dropout -> + residual -> LayerNorm over ragged rows, two launches of the implicit
GEMM of csrc/predictor.hip), `ConvFeedForward`, the sublayer as a module, `FFTBlock` (self-attention + LayerNorm, then the
sublayer), `FFTStack` (a sinusoidal table, then blocks) and `FastSpeech2Student` (embedding -> FFTStack -> VarianceAdaptor ->
FFTStack -> mel head).  The feed-forward half reads nothing at or behind a length, gives an utterance alone the bits it has in a
batch, and takes every sum in a fixed order; the attention half inherits the contract of `ops` (see `FFTBlock`).  Nothing is read
back to the host, and there is no CPU fallback."""
from __future__ import annotations

import math

import torch
from torch import nn

from .predictor import KernelVariancePredictor, _drop, _param
from .variance import VarianceAdaptor, _lens

MAX_ROWS = 4096              # RC_MAX_P of csrc/predictor.hip: phonemes or frames of one utterance
MAX_D = 256                  # RC_COLS: the LayerNorm epilogue owns a whole row
MAX_HIDDEN = 1024            # RC_MAX_CIN: the reduction depth of the second convolution
MAX_TAPS = 9                 # RC_MAX_TAPS

__all__ = ["ragged_conv_ffn", "ConvFeedForward", "FFTBlock", "FFTStack", "FastSpeech2Student"]


# ------------------------------------------------------------------------------------------------ checks
def _rows(x, fn):
    """(B, Pmax, D) fp32 on the device, handed on through its strides when they allow float4 rows -> x, ld_row, ld_batch"""
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{fn}: x must be (B, Pmax, D), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise ValueError(f"{fn}.x: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {x.device}")
    if x.dtype != torch.float32:
        raise ValueError(f"{fn}.x: expected dtype {torch.float32}, got {x.dtype}")
    B, Pmax, D = x.shape
    if D % 32 != 0 or not 32 <= D <= MAX_D:
        raise ValueError(f"{fn}: D must be a multiple of 32 in [32, {MAX_D}], got {D}")
    if Pmax > MAX_ROWS:
        raise ValueError(f"{fn}: Pmax must be in [1, {MAX_ROWS}] rows, got {Pmax}")
    if B > 65535:
        raise ValueError(f"{fn}: B must be in [1, 65535], got {B}")
    ok = x.stride(2) == 1 and x.data_ptr() % 16 == 0
    ok = ok and (Pmax == 1 or (x.stride(1) >= D and x.stride(1) % 4 == 0))
    ld_row = x.stride(1) if Pmax > 1 else D
    ok = ok and (B == 1 or (x.stride(0) % 4 == 0 and x.stride(0) >= (Pmax - 1) * ld_row + D))
    if not ok:
        x = x.contiguous()
        ld_row = D
    return x, ld_row, (x.stride(0) if B > 1 else Pmax * ld_row)


def _taps(k, fn, name):
    if isinstance(k, bool) or not isinstance(k, int) or k % 2 == 0 or not 1 <= k <= MAX_TAPS:
        raise ValueError(f"{fn}: {name} must be odd in [1, {MAX_TAPS}], got {k!r}")
    return k


def _widths(d_model, d_hidden, fn):
    if isinstance(d_model, bool) or not isinstance(d_model, int) or d_model % 32 != 0 or not 32 <= d_model <= MAX_D:
        raise ValueError(f"{fn}: d_model must be a multiple of 32 in [32, {MAX_D}], got {d_model!r}")
    if isinstance(d_hidden, bool) or not isinstance(d_hidden, int) or d_hidden % 32 != 0 or not 32 <= d_hidden <= MAX_HIDDEN:
        raise ValueError(f"{fn}: d_hidden must be a multiple of 32 in [32, {MAX_HIDDEN}], got {d_hidden!r}")


# ------------------------------------------------------------------------------------------------ the sublayer
class _RaggedConvFFN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ld_row, ld_batch, lens, w1, b1, w2, b2, gamma, beta, eps, drop_p, seed):
        from . import _lib
        from .ops import _p, _ss, _stream
        B, Pmax, D = x.shape
        Chid, _, k1 = w1.shape
        k2 = w2.shape[2]
        dev = x.device
        grads = any(ctx.needs_input_grad)
        wgrads = any(ctx.needs_input_grad[4:8])
        y = torch.empty(B, Pmax, D, dtype=torch.float32, device=dev)
        h = torch.empty(B, Pmax, Chid, dtype=torch.float32, device=dev)
        s = torch.empty(B, Pmax, D, dtype=torch.float32, device=dev) if grads else None
        mean = torch.empty(B, Pmax, dtype=torch.float32, device=dev) if grads else None
        rstd = torch.empty(B, Pmax, dtype=torch.float32, device=dev) if grads else None
        xm = torch.empty(B, Pmax, D, dtype=torch.float32, device=dev) if wgrads else None
        ss = _ss()
        _lib.check(_lib.load().ttts_ragged_conv_ffn_fwd(_p(x), ld_row, ld_batch, _p(lens), _p(w1), _p(b1), _p(w2), _p(b2), _p(gamma),
                                                        _p(beta), B, Pmax, D, Chid, k1, k2, eps, drop_p, seed, ss, _p(h), _p(y), _p(s),
                                                        _p(mean), _p(rstd), _p(xm), _stream()), "ttts_ragged_conv_ffn_fwd")
        if grads:
            ctx.save_for_backward(s, mean, rstd, h, xm, lens, w1, w2, gamma)
        ctx.shape = (B, Pmax, D, Chid, k1, k2)
        ctx.drop = (drop_p, seed, ss)      # backward regenerates the dropout mask under the step-state word of ITS forward
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import _lib
        from .ops import _p, _stream, _ws
        lib = _lib.load()
        s, mean, rstd, h, xm, lens, w1, w2, gamma = ctx.saved_tensors
        B, Pmax, D, Chid, k1, k2 = ctx.shape
        drop_p, seed, ss = ctx.drop
        dev = dy.device
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        dx = torch.empty(B, Pmax, D, dtype=torch.float32, device=dev) if need[0] else None
        dw1 = db1 = dw2 = db2 = None
        if xm is not None:
            dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
            db1, db2 = torch.empty(Chid, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        dgamma, dbeta = (torch.empty(D, dtype=torch.float32, device=dev) for _ in range(2))
        ws = _ws(lib.ttts_ragged_conv_ffn_workspace_bytes(B, Pmax, D, Chid, k1, k2), dev)
        _lib.check(lib.ttts_ragged_conv_ffn_bwd(_p(dy), _p(s), _p(mean), _p(rstd), _p(h), _p(xm), _p(lens), _p(w1), _p(w2), _p(gamma), B, Pmax,
                                                D, Chid, k1, k2, drop_p, seed, ss, _p(dx), _p(dw1), _p(db1), _p(dw2), _p(db2), _p(dgamma),
                                                _p(dbeta), _p(ws), ws.numel() * 4, 0, _stream()), "ttts_ragged_conv_ffn_bwd")
        return (dx, None, None, None, dw1 if need[4] else None, db1 if need[5] else None, dw2 if need[6] else None,
                db2 if need[7] else None, dgamma if need[8] else None, dbeta if need[9] else None, None, None, None)


def ragged_conv_ffn(x, lens, w1, b1, w2, b2, gamma, beta, eps=1e-5, drop_p=0.0, seed=0, training=True):
    """LayerNorm(x' + Dropout(Conv1d(ReLU(Conv1d(x'))))) over the rows of ragged utterances, two launches (csrc/predictor.hip).  x
    (B, Pmax, D) fp32, a strided view goes through its strides; lens (B,) integers; w1 (Chid, D, k1), b1 (Chid,), w2 (D, Chid, k2),
    b2 (D,) as two `nn.Conv1d` hold them (k odd, padding k // 2); gamma, beta (D,) as `nn.LayerNorm` -> (B, Pmax, D).  Rows at or
    behind lens[b] count as zeros for the taps and for the residual (their memory is not read: a NaN there does not leak) and are
    exact zeros in the result and in the gradient of x.  drop_p > 0 with training=True drops elements of the branch, before the
    residual add, by the counter-based hash of the flat output index under `seed` (`ops.seeds.next()` per call, as every dropout
    site of `ops`) and the active step state; training=False ignores drop_p.  D a multiple of 32 up to 256, Chid a multiple of 32
    up to 1024, k1 and k2 odd up to 9."""
    fn = "ragged_conv_ffn"
    x, ld_row, ld_batch = _rows(x, fn)
    B, Pmax, D = x.shape
    lens = _lens(lens, B, fn, "lens", x.device)
    if w1.dim() != 3 or w1.size(1) != D:
        raise ValueError(f"{fn}: w1 must be (Chid, {D}, k1), got {tuple(w1.shape)}")
    Chid, _, k1 = w1.shape
    if Chid % 32 != 0 or not 32 <= Chid <= MAX_HIDDEN:
        raise ValueError(f"{fn}: Chid must be a multiple of 32 in [32, {MAX_HIDDEN}], got {Chid}")
    if w2.dim() != 3 or w2.size(0) != D or w2.size(1) != Chid:
        raise ValueError(f"{fn}: w2 must be ({D}, {Chid}, k2), got {tuple(w2.shape)}")
    k2 = w2.size(2)
    for k in (k1, k2):
        if k % 2 == 0 or not 1 <= k <= MAX_TAPS:
            raise ValueError(f"{fn}: the kernel sizes must be odd in [1, {MAX_TAPS}], got {k}")
    w1, w2 = _param(w1, (Chid, D, k1), fn, "w1"), _param(w2, (D, Chid, k2), fn, "w2")
    b1 = _param(b1, (Chid,), fn, "b1")
    b2, gamma, beta = (_param(t, (D,), fn, name) for t, name in ((b2, "b2"), (gamma, "gamma"), (beta, "beta")))
    eps = float(eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"{fn}: eps must be positive and finite, got {eps}")
    drop_p = _drop(drop_p, fn) if training else 0.0
    return _RaggedConvFFN.apply(x, ld_row, ld_batch, lens, w1, b1, w2, b2, gamma, beta, eps, drop_p, int(seed) & 0xFFFFFFFFFFFFFFFF)


class ConvFeedForward(nn.Module):
    """`ragged_conv_ffn` as a module: `w_1`, `w_2` (two `nn.Conv1d` that hold the weights; their own forward is not used) and
    `layer_norm` (an `nn.LayerNorm`), so the parameters carry the usual names and shapes.  (x (B, Pmax, d_model), lens) -> (B,
    Pmax, d_model)."""

    def __init__(self, d_model, d_hidden, kernel_sizes=(9, 1), dropout=0.0):
        super().__init__()
        fn = "ConvFeedForward"
        _widths(d_model, d_hidden, fn)
        if len(tuple(kernel_sizes)) != 2:
            raise ValueError(f"{fn}: kernel_sizes must be two odd sizes, got {kernel_sizes!r}")
        k1, k2 = (_taps(k, fn, "kernel_sizes") for k in kernel_sizes)
        self.w_1 = nn.Conv1d(d_model, d_hidden, k1, padding=k1 // 2)
        self.w_2 = nn.Conv1d(d_hidden, d_model, k2, padding=k2 // 2)
        self.layer_norm = nn.LayerNorm(d_model)
        self.dropout = _drop(dropout, fn)

    def forward(self, x, lens):
        from . import ops
        p = self.dropout if self.training else 0.0
        return ragged_conv_ffn(x, lens, self.w_1.weight, self.w_1.bias, self.w_2.weight, self.w_2.bias, self.layer_norm.weight,
                               self.layer_norm.bias, eps=self.layer_norm.eps, drop_p=p, seed=ops.seeds.next() if p > 0 else 0)


# ------------------------------------------------------------------------------------------------ block, stack
class _MaskRows(torch.autograd.Function):
    """a copy of x (B, T, C) with exact zeros at and behind lens[b] (ttts_mask_rows); the gradient alike"""

    @staticmethod
    def forward(ctx, x, lens):
        ctx.save_for_backward(lens)
        return _MaskRows._masked(x, lens)

    @staticmethod
    def _masked(x, lens):
        from . import _lib
        from .ops import _p, _stream
        y = x.detach().clone(memory_format=torch.contiguous_format)
        B, T, C = y.shape
        _lib.check(_lib.load().ttts_mask_rows(_p(y), _p(lens), B, 1, T, C, _stream()), "ttts_mask_rows")
        return y

    @staticmethod
    def backward(ctx, dy):
        return _MaskRows._masked(dy, ctx.saved_tensors[0]), None


class FFTBlock(nn.Module):
    """One feed-forward Transformer block of FastSpeech (post-norm): LayerNorm(x + Dropout(SelfAttention(x))) under the length
    mask, then `ragged_conv_ffn`.  (x (B, Pmax, d_model), lens (B,)) -> (B, Pmax, d_model), exact zeros behind the lengths.
    The attention half is `MultiheadAttention.self_attention` + `ops.layer_norm` and inherits their contract: x must be finite
    everywhere (rows behind a length too), and the fp16x3 projections scale by measured maxima, so an utterance's bits may depend
    on its batch.  Heads of up to 128 columns run on the attention kernels; head_dim > 128 falls to `ops.masked_attention` (tensor
    algebra), as everywhere in `ops`.  The feed-forward half reads nothing behind a length (no mask launch between the halves) and
    gives an utterance alone the bits it has in the batch, given the same input rows."""

    def __init__(self, d_model=256, n_head=2, d_hidden=1024, kernel_sizes=(9, 1), dropout=0.2):
        super().__init__()
        from .model.layers import MultiheadAttention
        _widths(d_model, d_hidden, "FFTBlock")
        self.dropout = _drop(dropout, "FFTBlock")
        self.self_attn = MultiheadAttention(d_model, n_head, dropout=self.dropout)
        self.norm = nn.LayerNorm(d_model)
        self.ffn = ConvFeedForward(d_model, d_hidden, kernel_sizes, self.dropout)

    def forward(self, x, lens):
        from . import ops
        lens = _lens(lens, x.size(0), "FFTBlock", "lens", x.device)
        p = self.dropout if self.training else 0.0
        s = self.self_attn.self_attention(x, lens, False, residual=x, out_drop=p)
        return self.ffn(ops.layer_norm(s, self.norm.weight, self.norm.bias, self.norm.eps), lens)


def _sinusoids(max_len, d_model):
    pos = torch.arange(max_len, dtype=torch.float64)[:, None]
    inv = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float64) * (-math.log(10000.0) / d_model))
    pe = torch.zeros(max_len, d_model, dtype=torch.float64)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * inv), torch.cos(pos * inv)
    return pe.to(torch.float32)


class FFTStack(nn.Module):
    """n_layers `FFTBlock`s behind a fixed sinusoidal position table: x + pe[:Pmax] (`ops.posenc` with a constant alpha of 1 and
    no dropout), rows behind the lengths zeroed (`ttts_mask_rows`), then the blocks.  (x (B, Pmax, d_model), lens) -> (B, Pmax,
    d_model), zeros behind the lengths.  x must be finite everywhere (see `FFTBlock`).  The table and alpha are buffers kept out
    of the `state_dict`."""

    def __init__(self, n_layers, d_model=256, n_head=2, d_hidden=1024, kernel_sizes=(9, 1), dropout=0.2, max_len=MAX_ROWS):
        super().__init__()
        if isinstance(n_layers, bool) or not isinstance(n_layers, int) or n_layers < 1:
            raise ValueError(f"FFTStack: n_layers must be a positive integer, got {n_layers!r}")
        if isinstance(max_len, bool) or not isinstance(max_len, int) or not 1 <= max_len <= MAX_ROWS:
            raise ValueError(f"FFTStack: max_len must be an integer in [1, {MAX_ROWS}] rows, got {max_len!r}")
        self.layers = nn.ModuleList(FFTBlock(d_model, n_head, d_hidden, kernel_sizes, dropout) for _ in range(n_layers))
        self.max_len = max_len
        self.register_buffer("pe", _sinusoids(max_len, d_model), persistent=False)
        self.register_buffer("alpha", torch.ones(1), persistent=False)

    def forward(self, x, lens):
        from . import ops
        if x.dim() != 3 or x.size(1) > self.max_len:
            raise ValueError(f"FFTStack: x must be (B, Pmax <= {self.max_len}, d_model), got {tuple(x.shape)}")
        lens = _lens(lens, x.size(0), "FFTStack", "lens", x.device)
        x = _MaskRows.apply(ops.posenc(x, self.pe, self.alpha, 0.0, 0), lens)
        for layer in self.layers:
            x = layer(x, lens)
        return x


# ------------------------------------------------------------------------------------------------ the student
class FastSpeech2Student(nn.Module):
    """A FastSpeech-2 student on the library's kernels: `ops.embedding` -> `FFTStack` over the phonemes -> `VarianceAdaptor` ->
    `FFTStack` over the frames with the adaptor's `mel_lens` -> `ops.linear` to n_mels.  forward(phoneme (B, Pmax) int64,
    phoneme_lens (B,), durations, pitch, energy, max_len, d_control, p_control, e_control) returns the adaptor's dict plus 'melspec'
    (B, T, n_mels), exact zeros behind mel_lens.  With targets it is the training forward; without them it synthesises from its
    own predictions, and an eval call with a fixed max_len captures into one HIP graph.  `predictor`: what `VarianceAdaptor`
    takes; further keywords go to the adaptor.  decoder_layers is 6 in the paper.  No post-net, no speakers."""

    def __init__(self, n_vocab, d_model=256, encoder_layers=4, decoder_layers=4, n_head=2, d_hidden=1024, kernel_sizes=(9, 1), n_mels=80,
                 dropout=0.2, predictor=KernelVariancePredictor, **adaptor_kw):
        super().__init__()
        fn = "FastSpeech2Student"
        if isinstance(n_vocab, bool) or not isinstance(n_vocab, int) or n_vocab < 1:
            raise ValueError(f"{fn}: n_vocab must be a positive integer, got {n_vocab!r}")
        if isinstance(n_mels, bool) or not isinstance(n_mels, int) or n_mels < 4 or n_mels % 4 != 0:
            raise ValueError(f"{fn}: n_mels must be a positive multiple of 4, got {n_mels!r}")
        _widths(d_model, d_hidden, fn)
        self.embedding = nn.Embedding(n_vocab, d_model)
        self.encoder = FFTStack(encoder_layers, d_model, n_head, d_hidden, kernel_sizes, dropout)
        self.adaptor = VarianceAdaptor(d_model, predictor=predictor, **adaptor_kw)
        self.decoder = FFTStack(decoder_layers, d_model, n_head, d_hidden, kernel_sizes, dropout)
        self.mel_linear = nn.Linear(d_model, n_mels)

    def forward(self, phoneme, phoneme_lens, durations=None, pitch=None, energy=None, max_len=None, d_control=1.0, p_control=1.0,
                e_control=1.0):
        from . import ops
        fn = "FastSpeech2Student"
        if phoneme.dim() != 2 or phoneme.dtype != torch.int64:
            raise ValueError(f"{fn}: phoneme must be (B, Pmax) int64, got {tuple(phoneme.shape)} {phoneme.dtype}")
        lens = _lens(phoneme_lens, phoneme.size(0), fn, "phoneme_lens", phoneme.device)
        x = self.encoder(ops.embedding(phoneme, self.embedding.weight), lens)
        out = self.adaptor(x, lens, durations=durations, pitch=pitch, energy=energy, max_len=max_len, d_control=d_control,
                           p_control=p_control, e_control=e_control)
        frames = out["frames"]
        if frames.size(1) > self.decoder.max_len:
            raise ValueError(f"{fn}: the decoder takes up to {self.decoder.max_len} frames, got {frames.size(1)}; pass max_len")
        y = self.decoder(frames, out["mel_lens"])
        mel = ops.linear(y, self.mel_linear.weight, self.mel_linear.bias)
        out["melspec"] = _MaskRows.apply(mel, out["mel_lens"])
        return out
