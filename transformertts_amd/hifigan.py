"""A HiFi-GAN generator on the library's kernels (csrc/hifigan.hip): ragged mel batches to waveforms, inference only.
`HiFiGANConfig` (the presets V1 and V3, or a `config.json`), `fold_weight_norm` (any of the three spellings of a weight-normed state
dict to plain weight / bias, once, in fp64 on the host), `transposed_as_conv` (a ConvTranspose1d as a 3-tap convolution onto
stride x Cout columns), `ragged_dilated_conv` (the convolution kernel on its own) and `HiFiGANGenerator`, which returns the dict
`Vocoder.__call__` returns.  Every utterance is vocoded as if it were alone, each convolution zero-padded at the utterance's own
ends: nothing at or behind a length is read, an utterance alone has the bits it has in a batch, and every call gives the same
bits.  Nothing is read back to the host, and there is no CPU fallback."""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

MAX_TAPS = 11                # HG_MAX_TAPS of csrc/hifigan.hip
MAX_DILATION = 12            # HG_MAX_DIL
MAX_CHANNELS = 512           # HG_MAX_CIN
MAX_COLUMNS = 2048           # HG_MAX_COUT: stride x Cout of an upsampler
MAX_FRAMES = 4096
MAX_ROWS = 1 << 21           # HG_MAX_ROWS
LRELU_SLOPE = 0.1
TAIL_SLOPE = 0.01            # F.leaky_relu's default: the slope in front of conv_post

__all__ = ["HiFiGANConfig", "HiFiGANGenerator", "fold_weight_norm", "transposed_as_conv", "ragged_dilated_conv", "load_hifigan"]


# ------------------------------------------------------------------------------------------------ config
def _ints(v, fn, name):
    try:
        t = tuple(v)
    except TypeError:
        raise ValueError(f"{fn}: {name} must be a sequence of integers, got {v!r}") from None
    if not t or any(isinstance(i, bool) or not isinstance(i, int) for i in t):
        raise ValueError(f"{fn}: {name} must be a non-empty sequence of integers, got {v!r}")
    return t


@dataclass(frozen=True)
class HiFiGANConfig:
    """The generator's shape: `resblock` "1" or "2", the upsamplers' strides and kernel sizes, the width `upsample_initial_channel`
    in front of the first upsampler (halved by each), the resblocks' kernel sizes and dilations, `n_mels`."""
    resblock: str = "1"
    upsample_rates: Tuple[int, ...] = (8, 8, 2, 2)
    upsample_kernel_sizes: Tuple[int, ...] = (16, 16, 4, 4)
    upsample_initial_channel: int = 512
    resblock_kernel_sizes: Tuple[int, ...] = (3, 7, 11)
    resblock_dilation_sizes: Tuple[Tuple[int, ...], ...] = ((1, 3, 5), (1, 3, 5), (1, 3, 5))
    n_mels: int = 80

    def __post_init__(self):
        fn = "HiFiGANConfig"
        set_ = object.__setattr__
        set_(self, "resblock", str(self.resblock))
        if self.resblock not in ("1", "2"):
            raise ValueError(f"{fn}: resblock must be '1' or '2', got {self.resblock!r}")
        set_(self, "upsample_rates", _ints(self.upsample_rates, fn, "upsample_rates"))
        set_(self, "upsample_kernel_sizes", _ints(self.upsample_kernel_sizes, fn, "upsample_kernel_sizes"))
        set_(self, "resblock_kernel_sizes", _ints(self.resblock_kernel_sizes, fn, "resblock_kernel_sizes"))
        try:
            dil = tuple(_ints(d, fn, "resblock_dilation_sizes") for d in self.resblock_dilation_sizes)
        except TypeError:
            raise ValueError(f"{fn}: resblock_dilation_sizes must be a sequence of sequences, got {self.resblock_dilation_sizes!r}") from None
        set_(self, "resblock_dilation_sizes", dil)
        if len(self.upsample_rates) != len(self.upsample_kernel_sizes):
            raise ValueError(f"{fn}: upsample_rates and upsample_kernel_sizes must have one entry per stage, got "
                             f"{self.upsample_rates} and {self.upsample_kernel_sizes}")
        if len(dil) != len(self.resblock_kernel_sizes):
            raise ValueError(f"{fn}: resblock_dilation_sizes must have one entry per resblock kernel size, got {dil} for "
                             f"{self.resblock_kernel_sizes}")
        for u, k in zip(self.upsample_rates, self.upsample_kernel_sizes):
            _check_transposed(k, u, fn)
        for k in self.resblock_kernel_sizes:
            if k % 2 == 0 or not 1 <= k <= MAX_TAPS:
                raise ValueError(f"{fn}: resblock_kernel_sizes must be odd in [1, {MAX_TAPS}], got {k}")
        for d in dil:
            if any(not 1 <= i <= MAX_DILATION for i in d):
                raise ValueError(f"{fn}: resblock_dilation_sizes must be in [1, {MAX_DILATION}], got {d}")
        for name in ("upsample_initial_channel", "n_mels"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{fn}: {name} must be a positive integer, got {v!r}")
        if self.n_mels % 4 != 0 or not 4 <= self.n_mels <= 128:
            raise ValueError(f"{fn}: n_mels must be a multiple of 4 in [4, 128], got {self.n_mels}")
        c0 = self.upsample_initial_channel
        if c0 % (1 << len(self.upsample_rates)) != 0:
            raise ValueError(f"{fn}: upsample_initial_channel {c0} cannot be halved {len(self.upsample_rates)} times")
        for c in self.channels:
            if c % 32 != 0 or not 32 <= c <= MAX_CHANNELS:
                raise ValueError(f"{fn}: every stage's width must be a multiple of 32 in [32, {MAX_CHANNELS}], got {self.channels} "
                                 f"(upsample_initial_channel {c0}; the V2 preset, 128 down to 8 channels, is not supported)")
        for u, c in zip(self.upsample_rates, self.channels[1:]):
            if u * c > MAX_COLUMNS:
                raise ValueError(f"{fn}: an upsampler's stride x width may reach {MAX_COLUMNS} columns, got {u} x {c}")

    @property
    def channels(self) -> Tuple[int, ...]:
        """the width in front of the first upsampler and behind each"""
        return tuple(self.upsample_initial_channel >> i for i in range(len(self.upsample_rates) + 1))

    @property
    def hop(self) -> int:
        return math.prod(self.upsample_rates)

    @classmethod
    def v1(cls, n_mels: int = 80):
        return cls("1", (8, 8, 2, 2), (16, 16, 4, 4), 512, (3, 7, 11), ((1, 3, 5),) * 3, n_mels)

    @classmethod
    def v3(cls, n_mels: int = 80):
        return cls("2", (8, 8, 4), (16, 16, 8), 256, (3, 5, 7), ((1, 2), (2, 6), (3, 12)), n_mels)

    @classmethod
    def v2(cls, n_mels: int = 80):
        raise ValueError("HiFiGANConfig: the V2 preset (upsample_initial_channel 128, ending at 8 channels) is not supported: "
                         "every stage's width must be a multiple of 32")

    @classmethod
    def from_json(cls, path: str):
        """the keys of the usual `config.json` (`num_mels` for n_mels)"""
        with open(path) as f:
            c = json.load(f)
        keys = ("resblock", "upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock_kernel_sizes",
                "resblock_dilation_sizes")
        for k in keys:
            if k not in c:
                raise ValueError(f"HiFiGANConfig.from_json: {path} has no key {k!r}")
        return cls(*[c[k] for k in keys], int(c.get("num_mels", c.get("n_mels", 80))))

    def layer_names(self):
        """-> [(state-dict prefix, 'conv' or 'up')] of every layer, in the order the generator runs them"""
        names = [("conv_pre", "conv")]
        nk = len(self.resblock_kernel_sizes)
        for i in range(len(self.upsample_rates)):
            names.append((f"ups.{i}", "up"))
            for j in range(nk):
                for m in range(len(self.resblock_dilation_sizes[j])):
                    if self.resblock == "1":
                        names += [(f"resblocks.{i * nk + j}.convs1.{m}", "conv"), (f"resblocks.{i * nk + j}.convs2.{m}", "conv")]
                    else:
                        names.append((f"resblocks.{i * nk + j}.convs.{m}", "conv"))
        names.append(("conv_post", "conv"))
        return names


def _check_transposed(k, u, fn):
    if isinstance(k, bool) or isinstance(u, bool) or not isinstance(k, int) or not isinstance(u, int) or u < 1:
        raise ValueError(f"{fn}: an upsampler's kernel size and stride must be positive integers, got {k!r} and {u!r}")
    if k < u or k > 2 * u:
        raise ValueError(f"{fn}: an upsampler's kernel size must be in [stride, 2 stride] (three input rows per output row), got "
                         f"kernel {k}, stride {u}")
    if (k - u) % 2 != 0:
        raise ValueError(f"{fn}: an upsampler's kernel size minus its stride must be even (padding (k - u) / 2), got kernel {k}, "
                         f"stride {u}")


# ------------------------------------------------------------------------------------------------ weights
def fold_weight_norm(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """`weight_g` / `weight_v` or `parametrizations.weight.original0` / `original1` -> `weight` = g v / ||v|| (the norm over every
    axis but 0, as `weight_norm` takes it for both layer kinds), in fp64 on the host, returned as fp32; plain entries pass through."""
    out = {}
    for key, v in state_dict.items():
        for g_name, v_name in ((".weight_g", ".weight_v"), (".parametrizations.weight.original0", ".parametrizations.weight.original1")):
            if key.endswith(g_name):
                prefix = key[:-len(g_name)]
                if prefix + v_name not in state_dict:
                    raise KeyError(f"fold_weight_norm: {key} has no partner {prefix + v_name}")
                g, d = v.detach().cpu().double(), state_dict[prefix + v_name].detach().cpu().double()
                if g.dim() != d.dim() or g.shape[0] != d.shape[0] or g.numel() != d.shape[0]:
                    raise ValueError(f"fold_weight_norm: {key} must have shape ({d.shape[0]}, 1, ...), got {tuple(g.shape)}")
                norm = d.flatten(1).norm(dim=1).reshape(g.shape)
                out[prefix + ".weight"] = (g * d / norm).to(v.dtype if v.dtype == torch.float64 else torch.float32)
                break
            if key.endswith(v_name):
                prefix = key[:-len(v_name)]
                if prefix + g_name not in state_dict:
                    raise KeyError(f"fold_weight_norm: {key} has no partner {prefix + g_name}")
                break
        else:
            out[key] = v.detach().cpu()
    return out


def transposed_as_conv(weight: torch.Tensor, stride: int) -> torch.Tensor:
    """ConvTranspose1d's weight (Cin, Cout, k) with stride u and padding (k - u) / 2 -> the weight (u Cout, Cin, 3) of the Conv1d
    (padding 1) whose output (B, T, u Cout), read as (B, T u, Cout), is the transposed convolution's:
    W[r Cout + co, ci, j] = w[ci, co, r + pad - (j - 1) u], zero where that index leaves [0, k)."""
    if weight.dim() != 3:
        raise ValueError(f"transposed_as_conv: weight must be (Cin, Cout, k), got {tuple(weight.shape)}")
    cin, cout, k = weight.shape
    _check_transposed(k, stride, "transposed_as_conv")
    u, pad = stride, (k - stride) // 2
    W = weight.new_zeros(u * cout, cin, 3)
    for r in range(u):
        for j in range(3):
            idx = r + pad - (j - 1) * u
            if 0 <= idx < k:
                W[r * cout:(r + 1) * cout, :, j] = weight[:, :, idx].t()
    return W


def _relaid(weight: torch.Tensor) -> torch.Tensor:
    """Conv1d's (Cout, Cin, k) -> the kernel's (k, Cin, Cout)"""
    return weight.permute(2, 1, 0).contiguous()


# ------------------------------------------------------------------------------------------------ the kernel on its own
def _act(x, fn, name, width=None):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{fn}: {name} must be (B, Nmax, C), got {tuple(x.shape) if isinstance(x, torch.Tensor) else x!r}")
    if not x.is_cuda:
        raise ValueError(f"{fn}.{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got {x.device}")
    if x.dtype != torch.float32:
        raise ValueError(f"{fn}.{name}: expected dtype {torch.float32}, got {x.dtype}")
    if x.requires_grad:
        raise ValueError(f"{fn}.{name}: inference only, a tensor that requires grad is refused")
    if width is not None and x.size(2) != width:
        raise ValueError(f"{fn}: {name} must have {width} columns, got {x.size(2)}")
    return x.contiguous()


def _conv_shape(cin, cout, taps, dilation, fn):
    if not ((cin % 32 == 0 and 32 <= cin <= MAX_CHANNELS) or (cin % 4 == 0 and 4 <= cin <= 128)):
        raise ValueError(f"{fn}: Cin must be a multiple of 32 in [32, {MAX_CHANNELS}] or a multiple of 4 in [4, 128], got {cin}")
    if cout % 32 != 0 or not 32 <= cout <= MAX_COLUMNS:
        raise ValueError(f"{fn}: Cout must be a multiple of 32 in [32, {MAX_COLUMNS}], got {cout}")
    if taps % 2 == 0 or not 1 <= taps <= MAX_TAPS:
        raise ValueError(f"{fn}: taps must be odd in [1, {MAX_TAPS}], got {taps}")
    if isinstance(dilation, bool) or not isinstance(dilation, int) or not 1 <= dilation <= MAX_DILATION:
        raise ValueError(f"{fn}: dilation must be an integer in [1, {MAX_DILATION}], got {dilation!r}")


def _conv(x, lens, w, bias, residual, y, acc, taps, dilation, slope, acc_mode, scale):
    """ttts_hifigan_conv on checked operands; w is re-laid (taps, Cin, Cout)"""
    from . import _lib
    from .ops import _p, _stream
    B, N, cin = x.shape
    cout = w.shape[2]
    _lib.check(_lib.load().ttts_hifigan_conv(_p(x), _p(lens), _p(w), _p(bias), _p(residual), _p(y), _p(acc), B, N, cin, cout, taps,
                                             dilation, 1.0 if slope is None else slope, acc_mode, scale, _stream()),
               "ttts_hifigan_conv")


def ragged_dilated_conv(x, lens, weight, bias=None, dilation=1, in_slope=None, residual=None):
    """Conv1d(leaky_relu(x', in_slope)) + bias + residual over the rows of ragged utterances, one launch (csrc/hifigan.hip).  x (B,
    Nmax, Cin) fp32; lens (B,) integers; weight (Cout, Cin, taps) and bias (Cout,) as `nn.Conv1d` holds them, taps odd up to 11,
    padding dilation (taps // 2); residual (B, Nmax, Cout) -> (B, Nmax, Cout).  Rows at or behind lens[b] count as zeros, are not
    read, and are exact zeros in the result.  in_slope None: no activation.  Cin and Cout multiples of 32 up to 512 (Cin also a
    multiple of 4 up to 128; Cout up to 2048); dilation up to 12.  No autograd."""
    from .variance import _lens
    fn = "ragged_dilated_conv"
    x = _act(x, fn, "x")
    B, N, cin = x.shape
    if N > MAX_ROWS or B > 65535:
        raise ValueError(f"{fn}: x may hold up to 65535 utterances of {MAX_ROWS} rows, got {tuple(x.shape)}")
    lens = _lens(lens, B, fn, "lens", x.device)
    if not isinstance(weight, torch.Tensor) or weight.dim() != 3 or weight.size(1) != cin:
        raise ValueError(f"{fn}: weight must be (Cout, {cin}, taps), got {tuple(weight.shape)}")
    cout, _, taps = weight.shape
    _conv_shape(cin, cout, taps, dilation, fn)
    for t, name in ((weight, "weight"), (bias, "bias")):
        if t is not None and (t.requires_grad or t.dtype != torch.float32):
            raise ValueError(f"{fn}.{name}: expected fp32 without requires_grad (inference only), got {t.dtype}")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"{fn}: bias must be ({cout},), got {tuple(bias.shape)}")
    if residual is not None:
        residual = _act(residual, fn, "residual", cout)
        if residual.shape[:2] != x.shape[:2]:
            raise ValueError(f"{fn}: residual must be ({B}, {N}, {cout}), got {tuple(residual.shape)}")
    if in_slope is not None:
        in_slope = float(in_slope)
        if not math.isfinite(in_slope):
            raise ValueError(f"{fn}: in_slope must be finite, got {in_slope}")
    w = _relaid(weight.detach().to(x.device))
    bias = None if bias is None else bias.detach().to(x.device).contiguous()
    y = torch.empty(B, N, cout, dtype=torch.float32, device=x.device)
    _conv(x, lens, w, bias, residual, y, None, taps, dilation, in_slope, 0, 1.0)
    return y


# ------------------------------------------------------------------------------------------------ the generator
class HiFiGANGenerator:
    """A HiFi-GAN generator from a `state_dict` in any of the three spellings (`fold_weight_norm`), folded and re-laid once and kept
    on the device.  gen(melspec (B, Tmax, n_mels) fp32, mel_lens (B,)) -> {'wave': (B, Tmax hop) fp32, 'wave_lens': clamp(mel_lens,
    0, Tmax) hop}, what `Vocoder.__call__` returns; samples behind wave_lens are exact zeros.  `mean` / `std`: the mel is
    denormalised first (`denormalize`).  Up to 4096 frames.  A call whose largest activation would pass `max_bytes` (default: the
    kernels' operand limit) is split over the batch by shape alone, so a call with fixed shapes captures into one HIP graph."""

    def __init__(self, config: HiFiGANConfig, state_dict: Dict[str, torch.Tensor], device=None, mean=None, std=None):
        from . import _lib
        if not isinstance(config, HiFiGANConfig):
            raise ValueError(f"HiFiGANGenerator: config must be a HiFiGANConfig, got {type(config).__name__}")
        self.config = config
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise ValueError(f"HiFiGANGenerator: expected a CUDA/HIP device (the HIP path has no CPU fallback), got {self.device}")
        self.hop = config.hop
        self.max_operand_bytes = int(_lib.load().ttts_hifigan_max_operand_bytes())
        sd = fold_weight_norm(state_dict)
        ch = config.channels
        shapes = {"conv_pre": (ch[0], config.n_mels, 7), "conv_post": (1, ch[-1], 7)}
        nk = len(config.resblock_kernel_sizes)
        for i, (u, k) in enumerate(zip(config.upsample_rates, config.upsample_kernel_sizes)):
            shapes[f"ups.{i}"] = (ch[i], ch[i + 1], k)
            for j, kk in enumerate(config.resblock_kernel_sizes):
                for name, kind in config.layer_names():
                    if name.startswith(f"resblocks.{i * nk + j}."):
                        shapes[name] = (ch[i + 1], ch[i + 1], kk)
        self.layers = {}
        for name, kind in config.layer_names():                              # every key and shape, before anything goes to the device
            for part in ("weight", "bias"):
                if f"{name}.{part}" not in sd:
                    raise KeyError(f"HiFiGANGenerator: the state dict has no {name}.{part} (nor its weight-norm spellings)")
            w, b = sd[f"{name}.weight"], sd[f"{name}.bias"]
            if tuple(w.shape) != shapes[name] or tuple(b.shape) != (shapes[name][1 if kind == "up" else 0],):
                raise ValueError(f"HiFiGANGenerator: {name}.weight must be {shapes[name]}, got {tuple(w.shape)} (bias {tuple(b.shape)})")
        for name, kind in config.layer_names():
            w, b = sd[f"{name}.weight"].float(), sd[f"{name}.bias"].float()
            if kind == "up":
                u = config.upsample_rates[int(name.split(".")[1])]
                w, b = transposed_as_conv(w, u), b.repeat(u)
            self.layers[name] = (_relaid(w).to(self.device), b.contiguous().to(self.device), w.shape[2])
        self.mean = None if mean is None else torch.as_tensor(mean, dtype=torch.float32, device=self.device)
        self.std = None if std is None else torch.as_tensor(std, dtype=torch.float32, device=self.device)
        if (self.mean is None) != (self.std is None):
            raise ValueError("HiFiGANGenerator: mean and std go together")

    # -------------------------------------------------------------------------------------------- sizes
    def _widest(self, Tmax: int) -> int:
        """floats per utterance of the largest activation"""
        c, rows, best = self.config.channels, Tmax, Tmax * max(self.config.n_mels, self.config.channels[0])
        for i, u in enumerate(self.config.upsample_rates):
            rows *= u
            best = max(best, rows * c[i + 1])
        return best

    def peak_bytes(self, B: int, Tmax: int, max_bytes: Optional[int] = None) -> int:
        """bytes of intermediate buffers one call holds at its peak: the stage with the largest activation holds five of them
        (the stage's input, the running mean of its resblocks, a resblock's two alternating states and its inner activation;
        four with resblock "2"), over the utterances of one batch part"""
        part = self._part(B, Tmax, max_bytes)
        return (5 if self.config.resblock == "1" else 4) * part * self._widest(Tmax) * 4

    def _part(self, B, Tmax, max_bytes):
        limit = self.max_operand_bytes if max_bytes is None else int(max_bytes)
        per = self._widest(Tmax) * 4
        if per > limit:
            raise ValueError(f"HiFiGANGenerator: one utterance of {Tmax} frames needs an activation of {per} bytes, the limit is {limit}")
        return max(1, min(B, limit // per))

    # -------------------------------------------------------------------------------------------- the call
    def __call__(self, melspec, mel_lens, max_bytes: Optional[int] = None):
        from .audio import denormalize
        from .variance import _lens
        fn = "HiFiGANGenerator"
        cfg = self.config
        if not isinstance(melspec, torch.Tensor) or melspec.dim() != 3 or melspec.size(2) != cfg.n_mels or min(melspec.shape) < 1:
            raise ValueError(f"{fn}: melspec must be (B, Tmax, {cfg.n_mels}), got {tuple(melspec.shape)}")
        melspec = _act(melspec, fn, "melspec")
        B, Tmax, _ = melspec.shape
        if Tmax > MAX_FRAMES or B > 65535:
            raise ValueError(f"{fn}: up to 65535 utterances of {MAX_FRAMES} frames, got {tuple(melspec.shape)}")
        lens = _lens(mel_lens, B, fn, "mel_lens", self.device).clamp(0, Tmax)
        if self.mean is not None:
            melspec = denormalize(melspec, self.mean, self.std)
        wave = torch.empty(B, Tmax * self.hop, dtype=torch.float32, device=self.device)
        part = self._part(B, Tmax, max_bytes)
        for b0 in range(0, B, part):
            self._run(melspec[b0:b0 + part].contiguous(), lens[b0:b0 + part].contiguous(), wave[b0:b0 + part])
        return {"wave": wave, "wave_lens": lens * self.hop}

    def _run(self, mel, lens, wave):
        from . import _lib
        from .ops import _p, _stream, _ws
        cfg = self.config
        B, rows, _ = mel.shape
        ch = cfg.channels
        nk = len(cfg.resblock_kernel_sizes)

        def buf(n, c):
            return _ws(B * n * c * 4, self.device)[:B * n * c].view(B, n, c)

        w, b, k = self.layers["conv_pre"]
        x = buf(rows, ch[0])
        _conv(mel, lens, w, b, None, x, None, k, 1, None, 0, 1.0)
        for i, u in enumerate(cfg.upsample_rates):
            c = ch[i + 1]
            w, b, k = self.layers[f"ups.{i}"]
            up = buf(rows, u * c)
            _conv(x, lens, w, b, None, up, None, k, 1, LRELU_SLOPE, 0, 1.0)
            rows, lens = rows * u, lens * u                                  # (B, T, u C) row-major is (B, T u, C) row-major
            x = up.view(B, rows, c)
            mean, s0, s1 = buf(rows, c), buf(rows, c), buf(rows, c)
            t = buf(rows, c) if cfg.resblock == "1" else None
            for j, kk in enumerate(cfg.resblock_kernel_sizes):
                dils = cfg.resblock_dilation_sizes[j]
                prefix = f"resblocks.{i * nk + j}"
                cur = x
                for m, d in enumerate(dils):
                    last = m == len(dils) - 1
                    out = None if last else (s0 if cur is not s0 else s1)
                    mode = 0 if not last else 1 if j == 0 else 2             # the mean over the blocks, ascending, 1 / nk in the last
                    scale = 1.0 / nk if last and j == nk - 1 else 1.0
                    acc = mean if last else None
                    if cfg.resblock == "1":
                        w1, b1, _ = self.layers[f"{prefix}.convs1.{m}"]
                        w2, b2, _ = self.layers[f"{prefix}.convs2.{m}"]
                        _conv(cur, lens, w1, b1, None, t, None, kk, d, LRELU_SLOPE, 0, 1.0)
                        _conv(t, lens, w2, b2, cur, out, acc, kk, 1, LRELU_SLOPE, mode, scale)
                    else:
                        w1, b1, _ = self.layers[f"{prefix}.convs.{m}"]
                        _conv(cur, lens, w1, b1, cur, out, acc, kk, d, LRELU_SLOPE, mode, scale)
                    cur = out
            x = mean
            del up, mean, s0, s1, t, cur, out, acc                           # the next stage's buffers take their place
        w, b, k = self.layers["conv_post"]
        _lib.check(_lib.load().ttts_hifigan_post(_p(x), _p(lens), _p(w), _p(b), _p(wave), B, rows, ch[-1], k, TAIL_SLOPE, _stream()),
                   "ttts_hifigan_post")


def load_hifigan(path: str, config: HiFiGANConfig, **kw) -> HiFiGANGenerator:
    """a generator from a checkpoint file: `torch.load(path, map_location='cpu')`, its ['generator'] entry if there is one"""
    ckpt = torch.load(path, map_location="cpu")
    if isinstance(ckpt, dict) and "generator" in ckpt:
        ckpt = ckpt["generator"]
    return HiFiGANGenerator(config, ckpt, **kw)
