"""Reference of the HiFi-GAN generator (transformertts_amd/hifigan.py, csrc/hifigan.hip), written from the generator's description
as plain torch modules: usable in fp64 and fp32, with and without `weight_norm`.  `generate_per_utterance` runs every utterance
alone at its own length and pads the result with zeros: what the kernels compute on a ragged batch.  `dilated_conv_ref` is the
fp64 form of one ragged dilated convolution with its prologue and epilogue."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


def _wn(layer, spelling):
    if spelling == "plain":
        return layer
    if spelling == "weight_g":
        return torch.nn.utils.weight_norm(layer)
    if spelling == "parametrizations":
        return torch.nn.utils.parametrizations.weight_norm(layer)
    raise ValueError(spelling)


class ResBlock1(nn.Module):
    def __init__(self, c, k, dils, spelling):
        super().__init__()
        self.convs1 = nn.ModuleList(_wn(nn.Conv1d(c, c, k, dilation=d, padding=d * (k // 2)), spelling) for d in dils)
        self.convs2 = nn.ModuleList(_wn(nn.Conv1d(c, c, k, padding=k // 2), spelling) for _ in dils)

    def forward(self, x):
        for c1, c2 in zip(self.convs1, self.convs2):
            x = x + c2(F.leaky_relu(c1(F.leaky_relu(x, 0.1)), 0.1))
        return x


class ResBlock2(nn.Module):
    def __init__(self, c, k, dils, spelling):
        super().__init__()
        self.convs = nn.ModuleList(_wn(nn.Conv1d(c, c, k, dilation=d, padding=d * (k // 2)), spelling) for d in dils)

    def forward(self, x):
        for c in self.convs:
            x = x + c(F.leaky_relu(x, 0.1))
        return x


class Generator(nn.Module):
    """cfg: anything with the fields of HiFiGANConfig.  forward(mel (B, n_mels, T)) -> (B, T hop): torch's channel-first layout."""

    def __init__(self, cfg, spelling="plain", tail_slope=0.01):
        super().__init__()
        c0 = cfg.upsample_initial_channel
        self.nk = len(cfg.resblock_kernel_sizes)
        self.tail_slope = tail_slope
        self.conv_pre = _wn(nn.Conv1d(cfg.n_mels, c0, 7, padding=3), spelling)
        self.ups = nn.ModuleList()
        self.resblocks = nn.ModuleList()
        block = ResBlock1 if str(cfg.resblock) == "1" else ResBlock2
        for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            self.ups.append(_wn(nn.ConvTranspose1d(c0 >> i, c0 >> (i + 1), k, u, padding=(k - u) // 2), spelling))
            for kk, d in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
                self.resblocks.append(block(c0 >> (i + 1), kk, d, spelling))
        self.conv_post = _wn(nn.Conv1d(c0 >> len(cfg.upsample_rates), 1, 7, padding=3), spelling)

    def forward(self, x):
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            x = up(F.leaky_relu(x, 0.1))
            xs = self.resblocks[i * self.nk](x)
            for j in range(1, self.nk):
                xs = xs + self.resblocks[i * self.nk + j](x)
            x = xs / self.nk
        return torch.tanh(self.conv_post(F.leaky_relu(x, self.tail_slope))).squeeze(1)


def fan_in_state(cfg, seed, post_gain=1.0, spelling="plain"):
    """a state dict of `Generator(cfg, spelling)` in fp32 with weights randn / sqrt(Cin k) (for the transposed layers Cin k / stride:
    the taps one output row meets), biases 0.1 randn, conv_post's weight times post_gain; weight-norm spellings carry g = ||v||
    times a factor in [0.5, 1.5], so that the fold is not the identity"""
    g = torch.Generator().manual_seed(seed)
    m = Generator(cfg, "plain")
    sd = {}
    for name, p in m.state_dict().items():
        if name.endswith(".weight"):
            fan = p.shape[1] * p.shape[2]
            if name.startswith("ups."):
                fan = p.shape[0] * p.shape[2] / cfg.upsample_rates[int(name.split(".")[1])]
            w = torch.randn(p.shape, generator=g) / np.sqrt(fan)
            if name == "conv_post.weight":
                w = w * post_gain
            sd[name] = w
        else:
            sd[name] = 0.1 * torch.randn(p.shape, generator=g)
    if spelling == "plain":
        return sd
    names = {"weight_g": ("weight_g", "weight_v"), "parametrizations": ("parametrizations.weight.original0", "parametrizations.weight.original1")}[spelling]
    out = {}
    for name, p in sd.items():
        if name.endswith(".weight"):
            prefix = name[:-len("weight")]
            v = p * (0.5 + torch.rand((), generator=g))                      # any multiple of v gives the same direction
            gain = p.flatten(1).norm(dim=1).reshape(-1, 1, 1)                # g = ||w||: the fold gives w back (to rounding)
            out[prefix + names[0]], out[prefix + names[1]] = gain, v
        else:
            out[name] = p
    return out


def generate_per_utterance(model, mel, lens, hop):
    """mel (B, Tmax, n_mels) in the model's dtype, rows at or behind lens[b] ignored -> (B, Tmax hop): every utterance alone at its
    own length, zeros behind it"""
    B, Tmax, _ = mel.shape
    wave = mel.new_zeros(B, Tmax * hop)
    with torch.no_grad():
        for b in range(B):
            n = max(0, min(int(lens[b]), Tmax))
            if n > 0:
                y = model(mel[b:b + 1, :n].transpose(1, 2))
                assert y.shape == (1, n * hop)
                wave[b, :n * hop] = y[0]
    return wave


def dilated_conv_ref(x, lens, weight, bias=None, dilation=1, in_slope=None, residual=None):
    """fp64: x (B, Nmax, Cin), rows at or behind lens[b] ignored (they may hold NaN); weight (Cout, Cin, taps) as nn.Conv1d holds it
    -> (B, Nmax, Cout), zeros behind the lengths; every utterance alone, zero-padded at its own ends"""
    x = torch.as_tensor(x).double()
    w = torch.as_tensor(weight).double()
    B, N, _ = x.shape
    taps = w.shape[2]
    out = torch.zeros(B, N, w.shape[0], dtype=torch.float64)
    for b in range(B):
        n = max(0, min(int(lens[b]), N))
        if n == 0:
            continue
        xb = x[b, :n].t()[None]
        if in_slope is not None:
            xb = F.leaky_relu(xb, in_slope)
        y = F.conv1d(xb, w, None if bias is None else torch.as_tensor(bias).double(), dilation=dilation, padding=dilation * (taps // 2))[0].t()
        if residual is not None:
            y = y + torch.as_tensor(residual).double()[b, :n]
        out[b, :n] = y
    return out


def poison(lens, *arrays):
    """copies with NaN at and behind lens[b] along axis 1"""
    out = []
    for a in arrays:
        a = np.array(a, copy=True)
        for b, n in enumerate(lens):
            a[b, max(int(n), 0):] = np.nan
        out.append(a)
    return out[0] if len(out) == 1 else out
