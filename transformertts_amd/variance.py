"""Variance adaptor of a FastSpeech-2-style student on the kernels of csrc/variance.hip: the length regulator
(`length_regulate`, `LengthRegulator`), durations from predicted log-durations (`durations_from_log`), the quantised pitch and
energy embeddings (`variance_embed`, `VarianceEmbedding`, `variance_bins`), the three masked regression losses (`VarianceLoss`)
and `VarianceAdaptor`, which ties them to three predictors.  It consumes what `teacher_durations`, `PitchEnergy` and
`phoneme_average` produce.  Nothing here reads a value back to the host, except `length_regulate(max_len=None)`, which says so;
every sum is taken in a fixed order, so the same inputs give the same bits on every call.  There is no CPU fallback.

`VariancePredictor` is the one piece that is NOT on the library's kernels: a plain stock-torch module (correct, not tuned), a
few thousand phoneme rows per batch.  `predictor.KernelVariancePredictor` is the same module on kernels."""
from __future__ import annotations

import copy
import math

import torch
from torch import nn

MAX_PHONEMES = 4096          # VAR_MAX_P of csrc/variance.hip
MAX_FRAMES = 1 << 20         # VAR_MAX_T
MAX_WIDTH = 4096             # VAR_MAX_D
MAX_BINS = 4096              # VAR_MAX_BINS
MAX_TABLE_GRAD_WIDTH = 1024  # ttts_embedding_bwd (csrc/elementwise.hip)

__all__ = ["length_regulate", "LengthRegulator", "durations_from_log", "variance_embed", "VarianceEmbedding", "variance_bins",
           "VarianceLoss", "VariancePredictor", "VarianceAdaptor"]


# ------------------------------------------------------------------------------------------------ checks
def _rows(x, fn, name="x"):
    """(B, Pmax, D) fp32 on the device, handed on through its strides when they allow float4 rows -> x, ld_row, ld_batch"""
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{fn}: {name} must be (B, Pmax, D), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise ValueError(f"{fn}.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {x.device}")
    if x.dtype != torch.float32:
        raise ValueError(f"{fn}.{name}: expected dtype {torch.float32}, got {x.dtype}")
    B, Pmax, D = x.shape
    if D % 4 != 0 or D > MAX_WIDTH:
        raise ValueError(f"{fn}: D must be a multiple of 4 in [4, {MAX_WIDTH}], got {D}")
    if Pmax > MAX_PHONEMES:
        raise ValueError(f"{fn}: Pmax must be in [1, {MAX_PHONEMES}] phonemes, got {Pmax}")
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


def _lens(t, B, fn, name, device):
    if tuple(t.shape) != (B,):
        raise ValueError(f"{fn}.{name} must have shape ({B},), got {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{fn}.{name} must be integers, got {t.dtype}")
    return t.to(device).to(torch.int64).contiguous()


def _per_phoneme(t, B, Pmax, fn, name, dtype, device):
    if t.dim() != 2 or tuple(t.shape) != (B, Pmax):
        raise ValueError(f"{fn}: {name} must be ({B}, {Pmax}), got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{fn}.{name}: expected dtype {dtype}, got {t.dtype}")
    return t.detach().to(device).contiguous()


def _max_len(max_len, fn):
    if isinstance(max_len, bool) or not isinstance(max_len, int) or not 1 <= max_len <= MAX_FRAMES:
        raise ValueError(f"{fn}: max_len must be an integer in [1, 2^20] frames, got {max_len!r}")
    return max_len


# ------------------------------------------------------------------------------------------------ length regulator
class _LengthRegulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ld_row, ld_batch, durations, lens, Tmax):
        from . import _lib
        from .ops import _p, _stream
        B, Pmax, D = x.shape
        y = torch.empty(B, Tmax, D, dtype=torch.float32, device=x.device)
        mel_lens = torch.empty(B, dtype=torch.int64, device=x.device)
        index = torch.empty(B, Tmax, dtype=torch.int32, device=x.device)
        _lib.check(_lib.load().ttts_length_regulate_fwd(_p(x), ld_row, ld_batch, _p(durations), _p(lens), B, Pmax, Tmax, D, _p(y),
                                                        _p(mel_lens), _p(index), _stream()), "ttts_length_regulate_fwd")
        ctx.save_for_backward(durations, lens)
        ctx.shape = (B, Pmax, Tmax, D)
        ctx.mark_non_differentiable(mel_lens, index)
        return y, mel_lens, index

    @staticmethod
    def backward(ctx, dy, _dl, _di):
        from . import _lib
        from .ops import _p, _stream
        durations, lens = ctx.saved_tensors
        B, Pmax, Tmax, D = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty(B, Pmax, D, dtype=torch.float32, device=dy.device)
        _lib.check(_lib.load().ttts_length_regulate_bwd(_p(dy), _p(durations), _p(lens), B, Pmax, Tmax, D, _p(dx), 0, _stream()),
                   "ttts_length_regulate_bwd")
        return dx, None, None, None, None, None


def length_regulate(x, durations, phoneme_lens, max_len=None):
    """P phoneme rows -> T frame rows (csrc/variance.hip, one launch forward, one backward).  x (B, Pmax, D) fp32, a strided view
    goes through its strides; durations (B, Pmax) int64 as `teacher_durations` returns them (negative counts as 0, nothing at
    or behind phoneme_lens[b] is read); phoneme_lens (B,) integers -> {'frames': (B, max_len, D), 'mel_lens': (B,) int64,
    'index': (B, max_len) int32}.  Row t of utterance b is the row of the phoneme whose span [c_p, c_p + dur_p) holds t;
    rows from mel_lens[b] = min(sum dur, max_len) on are zeros and their index -1.  The gradient of x is the sum of the
    frame gradients of each phoneme in ascending t: bit for bit a sequential fp32 loop.
    max_len=None is allowed outside a graph capture only: it reads the longest sum of durations back to the host, the one
    host read of this module."""
    fn = "length_regulate"
    x, ld_row, ld_batch = _rows(x, fn)
    B, Pmax, _ = x.shape
    durations = _per_phoneme(durations, B, Pmax, fn, "durations", torch.int64, x.device)
    lens = _lens(phoneme_lens, B, fn, "phoneme_lens", x.device)
    if max_len is None:
        if torch.cuda.is_current_stream_capturing():
            raise ValueError(f"{fn}: max_len=None reads the durations back to the host and cannot be captured; pass max_len")
        valid = torch.arange(Pmax, device=x.device)[None, :] < lens[:, None]
        longest = int(torch.where(valid, durations.clamp(min=0, max=MAX_FRAMES), torch.zeros_like(durations)).sum(1).max())
        max_len = min(max(longest, 1), MAX_FRAMES)
    y, mel_lens, index = _LengthRegulate.apply(x, ld_row, ld_batch, durations, lens, _max_len(max_len, fn))
    return {"frames": y, "mel_lens": mel_lens, "index": index}


class LengthRegulator(nn.Module):
    """`length_regulate` as a module; `max_len` given here is the default of every call (a fixed one makes it capturable)."""

    def __init__(self, max_len=None):
        super().__init__()
        self.max_len = None if max_len is None else _max_len(max_len, "LengthRegulator")

    def forward(self, x, durations, phoneme_lens, max_len=None):
        return length_regulate(x, durations, phoneme_lens, self.max_len if max_len is None else max_len)


def durations_from_log(log_d, phoneme_lens, alpha=1.0, min_duration=0):
    """predicted log-durations -> integer durations at inference (one launch, nothing read back): d = max(0, rint((exp(log_d)
    - 1) * alpha)), halves to even as `torch.round`, evaluated in fp64; a NaN or infinite prediction gives 0; then at least
    min_duration for p < phoneme_lens[b]; 0 behind it.  log_d (B, Pmax) fp32 -> (B, Pmax) int64.  alpha > 1 slows down."""
    from . import _lib
    from .ops import _p, _stream
    fn = "durations_from_log"
    if log_d.dim() != 2 or min(log_d.shape) < 1:
        raise ValueError(f"{fn}: log_d must be (B, Pmax), got {tuple(log_d.shape)}")
    if not log_d.is_cuda:
        raise ValueError(f"{fn}.log_d: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {log_d.device}")
    if log_d.dtype != torch.float32:
        raise ValueError(f"{fn}.log_d: expected dtype {torch.float32}, got {log_d.dtype}")
    B, Pmax = log_d.shape
    if Pmax > MAX_PHONEMES:
        raise ValueError(f"{fn}: Pmax must be in [1, {MAX_PHONEMES}] phonemes, got {Pmax}")
    alpha = float(alpha)
    if not (alpha > 0.0 and math.isfinite(alpha)):
        raise ValueError(f"{fn}: alpha must be positive and finite, got {alpha}")
    if isinstance(min_duration, bool) or not isinstance(min_duration, int) or not 0 <= min_duration < (1 << 31):
        raise ValueError(f"{fn}: min_duration must be an integer in [0, 2^31 - 1], got {min_duration!r}")
    lens = _lens(phoneme_lens, B, fn, "phoneme_lens", log_d.device)
    log_d = log_d.detach().contiguous()
    out = torch.empty(B, Pmax, dtype=torch.int64, device=log_d.device)
    _lib.check(_lib.load().ttts_durations_from_log(_p(log_d), _p(lens), B, Pmax, alpha, min_duration, _p(out), _stream()),
               "ttts_durations_from_log")
    return out


# ------------------------------------------------------------------------------------------------ pitch / energy embeddings
def variance_bins(lo, hi, n_bins, scale="linear"):
    """the n_bins - 1 ascending fp32 boundaries between lo and hi that split the line into n_bins buckets, evenly ('linear') or
    evenly in the logarithm ('log', lo > 0); a value at or below lo falls into bucket 0, one above hi into bucket n_bins - 1.
    A host helper: a CPU tensor for `VarianceEmbedding`."""
    if isinstance(n_bins, bool) or not isinstance(n_bins, int) or not 2 <= n_bins <= MAX_BINS:
        raise ValueError(f"variance_bins: n_bins must be an integer in [2, {MAX_BINS}], got {n_bins!r}")
    if scale not in ("linear", "log"):
        raise ValueError(f"variance_bins: scale must be 'linear' or 'log', got {scale!r}")
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"variance_bins: need finite lo < hi (lo {lo}, hi {hi})")
    if scale == "log":
        if lo <= 0.0:
            raise ValueError(f"variance_bins: a log scale needs lo > 0, got {lo}")
        b = torch.linspace(math.log(lo), math.log(hi), n_bins - 1, dtype=torch.float64).exp()
    else:
        b = torch.linspace(lo, hi, n_bins - 1, dtype=torch.float64)
    return b.to(torch.float32)


def _bins(bins, n, name):
    bins = torch.as_tensor(bins)
    if bins.dim() != 1 or bins.numel() != n - 1:
        raise ValueError(f"VarianceEmbedding: {name} must hold n_bins - 1 = {n - 1} boundaries, got {tuple(bins.shape)}")
    bins = bins.detach().to(torch.float32)
    if bool(torch.isnan(bins).any()) or (n > 2 and bool((bins[1:] < bins[:-1]).any())):
        raise ValueError(f"VarianceEmbedding: {name} must be ascending and free of NaN")
    return bins.contiguous()


class _VarianceEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ld_row, ld_batch, lens, pitch, pitch_bins, pitch_table, energy, energy_bins, energy_table):
        from . import _lib
        from .ops import _p, _stream
        B, Pmax, D = x.shape
        y = torch.empty(B, Pmax, D, dtype=torch.float32, device=x.device)
        ids = [None if t is None else torch.empty(B, Pmax, dtype=torch.int64, device=x.device) for t in (pitch_table, energy_table)]
        n = [2 if t is None else t.size(0) for t in (pitch_table, energy_table)]
        _lib.check(_lib.load().ttts_variance_embed_fwd(_p(x), ld_row, ld_batch, _p(pitch), _p(energy), _p(pitch_bins), n[0],
                                                       _p(energy_bins), n[1], _p(pitch_table), _p(energy_table), _p(lens), B, Pmax, D,
                                                       _p(y), _p(ids[0]), _p(ids[1]), _stream()), "ttts_variance_embed_fwd")
        ctx.ids, ctx.n, ctx.d = ids, n, D
        ctx.tables = (pitch_table is not None, energy_table is not None)
        out = [y] + [t for t in ids if t is not None]
        ctx.mark_non_differentiable(*out[1:])
        return tuple(out)

    @staticmethod
    def backward(ctx, dy, *_):
        from . import _lib
        from .ops import _p, _stream
        dy = dy.contiguous()
        grads = []
        for k in range(2):                     # the table gradients: ttts_embedding_bwd on the saved ids (-1 matches no row)
            g = None
            if ctx.tables[k] and ctx.needs_input_grad[6 + 3 * k]:
                g = torch.empty(ctx.n[k], ctx.d, dtype=torch.float32, device=dy.device)
                _lib.check(_lib.load().ttts_embedding_bwd(_p(ctx.ids[k]), _p(dy), _p(g), ctx.ids[k].numel(), ctx.n[k], ctx.d, 0,
                                                          _stream()), "ttts_embedding_bwd")
            grads.append(g)
        return dy, None, None, None, None, None, grads[0], None, None, grads[1]


def variance_embed(x, phoneme_lens, pitch=None, pitch_bins=None, pitch_table=None, energy=None, energy_bins=None, energy_table=None):
    """y = (x + pitch_table[i]) + energy_table[j] in that order for p < phoneme_lens[b], y = x behind it (one launch).  i =
    torch.bucketize(pitch, pitch_bins): the number of boundaries strictly below the value; j alike.  x (B, Pmax, D) fp32 through
    its strides, pitch / energy (B, Pmax) fp32, the boundaries (n - 1,) ascending fp32, the tables (n, D) fp32.  Either feature
    may be absent (all three of its arguments None).  -> {'x': y, 'pitch_ids', 'energy_ids': (B, Pmax) int64, -1 behind the
    length, None for an absent feature}.  The gradient of x is dy itself; the table gradients come from `ttts_embedding_bwd`
    on the ids, in a fixed order."""
    fn = "variance_embed"
    x, ld_row, ld_batch = _rows(x, fn)
    B, Pmax, D = x.shape
    lens = _lens(phoneme_lens, B, fn, "phoneme_lens", x.device)
    feats = []
    for name, v, bins, table in (("pitch", pitch, pitch_bins, pitch_table), ("energy", energy, energy_bins, energy_table)):
        if v is None and bins is None and table is None:
            feats += [None, None, None]
            continue
        if v is None or bins is None or table is None:
            raise ValueError(f"{fn}: {name}, {name}_bins and {name}_table go together (all three or none)")
        v = _per_phoneme(v, B, Pmax, fn, name, torch.float32, x.device)
        if table.dim() != 2 or table.size(1) != D or not 2 <= table.size(0) <= MAX_BINS:
            raise ValueError(f"{fn}: {name}_table must be (n, {D}) with n in [2, {MAX_BINS}], got {tuple(table.shape)}")
        if not table.is_cuda or table.dtype != torch.float32:
            raise ValueError(f"{fn}.{name}_table: expected a {torch.float32} CUDA/HIP tensor, got {table.dtype} on {table.device}")
        if tuple(bins.shape) != (table.size(0) - 1,) or bins.dtype != torch.float32 or not bins.is_cuda:
            raise ValueError(f"{fn}: {name}_bins must be ({table.size(0) - 1},) {torch.float32} on the device, "
                             f"got {tuple(bins.shape)} {bins.dtype} on {bins.device}")
        if table.requires_grad and torch.is_grad_enabled() and D > MAX_TABLE_GRAD_WIDTH:
            raise ValueError(f"{fn}: the table gradient (ttts_embedding_bwd) takes D <= {MAX_TABLE_GRAD_WIDTH}, got {D}")
        feats += [v, bins.detach().contiguous(), table.contiguous()]
    out = _VarianceEmbed.apply(x, ld_row, ld_batch, lens, *feats)
    ids = list(out[1:])
    return {"x": out[0], "pitch_ids": ids.pop(0) if feats[2] is not None else None,
            "energy_ids": ids.pop(0) if feats[5] is not None else None}


class VarianceEmbedding(nn.Module):
    """The quantised pitch and energy embeddings of FastSpeech 2: boundaries as buffers, two tables as parameters.  A count of 0
    leaves a feature out.  Boundaries: `pitch_bins` / `energy_bins` (n - 1 ascending values, see `variance_bins`); the defaults
    are `PitchEnergy`'s F0 range on a log scale and [0, 1] on a linear one -- pass the ranges of your data."""

    def __init__(self, n_pitch_bins, n_energy_bins, d_model, pitch_bins=None, energy_bins=None, device=None):
        super().__init__()
        if isinstance(d_model, bool) or not isinstance(d_model, int) or d_model < 4 or d_model % 4 != 0 or d_model > MAX_WIDTH:
            raise ValueError(f"VarianceEmbedding: d_model must be a multiple of 4 in [4, {MAX_WIDTH}], got {d_model!r}")
        self.d_model = d_model
        defaults = {"pitch": (65.0, 600.0, "log"), "energy": (0.0, 1.0, "linear")}
        for name, n, bins in (("pitch", n_pitch_bins, pitch_bins), ("energy", n_energy_bins, energy_bins)):
            if isinstance(n, bool) or not isinstance(n, int) or not (n == 0 or 2 <= n <= MAX_BINS):
                raise ValueError(f"VarianceEmbedding: n_{name}_bins must be 0 (no {name}) or in [2, {MAX_BINS}], got {n!r}")
            if n == 0:
                self.register_buffer(name + "_bins", None)
                self.register_parameter(name + "_table", None)
                continue
            b = _bins(variance_bins(*defaults[name][:2], n, defaults[name][2]) if bins is None else bins, n, name + "_bins")
            self.register_buffer(name + "_bins", b.to(device))
            table = torch.empty(n, d_model, dtype=torch.float32, device=device)
            nn.init.normal_(table, 0.0, d_model ** -0.5)
            self.register_parameter(name + "_table", nn.Parameter(table))

    def forward(self, x, phoneme_lens, pitch=None, energy=None, return_ids=False):
        kw = {}
        for name, v in (("pitch", pitch), ("energy", energy)):
            table = getattr(self, name + "_table")
            if v is not None and table is None:
                raise ValueError(f"VarianceEmbedding: {name} given, but the module was built without a {name} table")
            if v is not None:
                kw.update({name: v, name + "_bins": getattr(self, name + "_bins"), name + "_table": table})
        out = variance_embed(x, phoneme_lens, **kw)
        return out if return_ids else out["x"]


# ------------------------------------------------------------------------------------------------ losses
class _VarianceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_d, pitch_pred, energy_pred, durations, pitch, energy, lens, weights):
        from . import _lib
        from .ops import _p, _stream
        B, Pmax = log_d.shape
        out = torch.empty(4, dtype=torch.float32, device=log_d.device)
        _lib.check(_lib.load().ttts_variance_loss_fwd(_p(log_d), _p(durations), _p(pitch_pred), _p(pitch), _p(energy_pred), _p(energy),
                                                      _p(lens), B, Pmax, *weights, _p(out), _stream()), "ttts_variance_loss_fwd")
        ctx.save_for_backward(log_d, pitch_pred, energy_pred, durations, pitch, energy, lens)
        ctx.weights = weights
        return out

    @staticmethod
    def backward(ctx, gout):
        from . import _lib
        from .ops import _p, _stream
        log_d, pitch_pred, energy_pred, durations, pitch, energy, lens = ctx.saved_tensors
        B, Pmax = log_d.shape
        gout = gout.contiguous()
        g = [torch.empty_like(log_d) for _ in range(3)]
        _lib.check(_lib.load().ttts_variance_loss_bwd(_p(log_d), _p(durations), _p(pitch_pred), _p(pitch), _p(energy_pred), _p(energy),
                                                      _p(lens), B, Pmax, *ctx.weights, _p(gout), _p(g[0]), _p(g[1]), _p(g[2]),
                                                      _stream()), "ttts_variance_loss_bwd")
        return g[0], g[1], g[2], None, None, None, None, None


class VarianceLoss(nn.Module):
    """Three masked mean-squared errors in one launch (and one for their gradients): the log-duration prediction against
    log(durations + 1), the pitch and the energy predictions against their targets, each a mean over the sum(phoneme_lens) valid
    phonemes, exactly 0 when there is none.  `pred` is what `VarianceAdaptor` returns (its 'log_duration', 'pitch', 'energy').
    -> {'duration', 'pitch', 'energy', 'total'}, total = (w_d duration + w_p pitch) + w_e energy."""

    def __init__(self, weights=(1.0, 1.0, 1.0)):
        super().__init__()
        weights = tuple(float(w) for w in weights)
        if len(weights) != 3 or not all(math.isfinite(w) for w in weights):
            raise ValueError(f"VarianceLoss: weights must be three finite numbers (duration, pitch, energy), got {weights}")
        self.weights = weights

    def forward(self, pred, durations, pitch, energy, phoneme_lens):
        fn = "VarianceLoss"
        log_d = pred["log_duration"]
        if log_d.dim() != 2 or min(log_d.shape) < 1:
            raise ValueError(f"{fn}: pred['log_duration'] must be (B, Pmax), got {tuple(log_d.shape)}")
        if not log_d.is_cuda:
            raise ValueError(f"{fn}.log_duration: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {log_d.device}")
        B, Pmax = log_d.shape
        if Pmax > MAX_PHONEMES:
            raise ValueError(f"{fn}: Pmax must be in [1, {MAX_PHONEMES}] phonemes, got {Pmax}")
        preds = []
        for name in ("log_duration", "pitch", "energy"):
            t = pred[name]
            if tuple(t.shape) != (B, Pmax):
                raise ValueError(f"{fn}: pred[{name!r}] must be ({B}, {Pmax}), got {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"{fn}.{name}: expected dtype {torch.float32}, got {t.dtype}")
            preds.append(t.contiguous())
        durations = _per_phoneme(durations, B, Pmax, fn, "durations", torch.int64, log_d.device)
        pitch = _per_phoneme(pitch, B, Pmax, fn, "pitch", torch.float32, log_d.device)
        energy = _per_phoneme(energy, B, Pmax, fn, "energy", torch.float32, log_d.device)
        lens = _lens(phoneme_lens, B, fn, "phoneme_lens", log_d.device)
        out = _VarianceLoss.apply(*preds, durations, pitch, energy, lens, self.weights)
        return {"duration": out[0], "pitch": out[1], "energy": out[2], "total": out[3]}


# ------------------------------------------------------------------------------------------------ predictor, adaptor
class VariancePredictor(nn.Module):
    """STOCK TORCH, not the library's kernels: FastSpeech 2's predictor, Conv1d(k) -> ReLU -> LayerNorm -> Dropout twice, then
    Linear -> 1, zero behind the lengths.  (x (B, Pmax, D), phoneme_lens) -> (B, Pmax).  Correct, not tuned: a few thousand
    phoneme rows per batch.  Any module with this signature can take its place in `VarianceAdaptor`.
    The two `nn.Conv1d` hold the weights; the convolution itself is taken as one matrix product over the k shifted copies of
    the rows, because the convolution library's 256-channel solver does not give the same bits on two calls (measured: the
    last bit moves between two eager calls), and the adaptor promises the same bits on every call."""

    def __init__(self, d_model, hidden=256, kernel_size=3, dropout=0.5):
        super().__init__()
        if kernel_size < 1 or kernel_size % 2 == 0:
            raise ValueError(f"VariancePredictor: kernel_size must be odd and positive, got {kernel_size}")
        pad = kernel_size // 2
        self.conv1, self.conv2 = nn.Conv1d(d_model, hidden, kernel_size, padding=pad), nn.Conv1d(hidden, hidden, kernel_size, padding=pad)
        self.norm1, self.norm2 = nn.LayerNorm(hidden), nn.LayerNorm(hidden)
        self.drop = nn.Dropout(dropout)
        self.out = nn.Linear(hidden, 1)

    @staticmethod
    def _conv(conv, h):
        """conv(h.transpose(1, 2)).transpose(1, 2) for h (B, P, C): the taps side by side, one matrix product"""
        k, P = conv.kernel_size[0], h.size(1)
        hp = nn.functional.pad(h, (0, 0, k // 2, k // 2))
        taps = torch.cat([hp[:, i:i + P] for i in range(k)], dim=2)                        # (B, P, k C): tap-major
        return nn.functional.linear(taps, conv.weight.permute(0, 2, 1).reshape(conv.out_channels, -1), conv.bias)

    def forward(self, x, phoneme_lens):
        valid = torch.arange(x.size(1), device=x.device)[None, :] < phoneme_lens.to(x.device)[:, None]
        keep, zero = valid[:, :, None], x.new_zeros(())            # the padding (a NaN even) must not leak through the taps
        h = self.drop(self.norm1(torch.relu(self._conv(self.conv1, torch.where(keep, x, zero)))))
        h = self.drop(self.norm2(torch.relu(self._conv(self.conv2, torch.where(keep, h, zero)))))
        return self.out(h)[:, :, 0].masked_fill(~valid, 0.0)


class VarianceAdaptor(nn.Module):
    """FastSpeech 2's variance adaptor: three predictors read the encoder output x; pitch and energy (targets when given, else
    the predictions scaled by p_control / e_control) are quantised, embedded and added; the length regulator expands the sum by
    the durations (targets when given, else `durations_from_log` of the prediction with alpha = d_control).

    predictor: None -> `VariancePredictor` (stock torch); a module mapping (x, phoneme_lens) -> (B, Pmax), copied three times;
    or a callable d_model -> such a module, called three times.  `pitch_bins` / `energy_bins`: n_bins - 1 boundaries each.
    With a fixed max_len and no targets the whole call is capturable into one HIP graph."""

    def __init__(self, d_model, n_bins=256, predictor=None, pitch_bins=None, energy_bins=None, min_duration=0, max_len=None, device=None):
        super().__init__()
        if predictor is None:
            make = lambda: VariancePredictor(d_model)
        elif isinstance(predictor, nn.Module):
            make = lambda: copy.deepcopy(predictor)
        elif callable(predictor):
            make = lambda: predictor(d_model)
        else:
            raise ValueError(f"VarianceAdaptor: predictor must be None, a module or a callable d_model -> module, got {type(predictor)}")
        self.duration_predictor, self.pitch_predictor, self.energy_predictor = make(), make(), make()
        self.embedding = VarianceEmbedding(n_bins, n_bins, d_model, pitch_bins=pitch_bins, energy_bins=energy_bins)
        self.min_duration = min_duration
        self.max_len = None if max_len is None else _max_len(max_len, "VarianceAdaptor")
        if device is not None:
            self.to(device)

    def forward(self, x, phoneme_lens, durations=None, pitch=None, energy=None, max_len=None, d_control=1.0, p_control=1.0,
                e_control=1.0):
        log_d = self.duration_predictor(x, phoneme_lens)
        pitch_pred = self.pitch_predictor(x, phoneme_lens)
        energy_pred = self.energy_predictor(x, phoneme_lens)
        use_pitch = pitch if pitch is not None else (pitch_pred.detach() if p_control == 1.0 else pitch_pred.detach() * p_control)
        use_energy = energy if energy is not None else (energy_pred.detach() if e_control == 1.0 else energy_pred.detach() * e_control)
        h = self.embedding(x, phoneme_lens, pitch=use_pitch, energy=use_energy)
        if durations is None:
            durations = durations_from_log(log_d, phoneme_lens, alpha=d_control, min_duration=self.min_duration)
        out = length_regulate(h, durations, phoneme_lens, self.max_len if max_len is None else max_len)
        out.update({"log_duration": log_d, "pitch": pitch_pred, "energy": energy_pred, "durations": durations})
        return out
