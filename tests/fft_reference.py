"""Oracles of the conv feed-forward sublayer, the FFT block and the FastSpeech-2 student (csrc/predictor.hip,
transformertts_amd/fft.py), written from the definition in DESIGN.md 28 in stock torch.  `ffn_ref` is differentiable and
`ffn_bwd_ref` restates the backward formula by formula with the ReLU gate and the keep mask as INPUTS, so a test can hand it the
gate a kernel took.  `fft_block_ref`, `fft_stack_ref` and `student_ref` take a `state_dict` and work in the dtype and on the device
of its tensors: in fp64 on the CPU they are the oracle, in fp32 they are the stock-torch restatement whose error a test compares
the kernel path's with.  Test infrastructure, no GPU needed."""
import math

import numpy as np
import torch
from torch.nn import functional as F

from predictor_reference import poison, valid_mask  # noqa: F401 -- `poison` puts NaN behind every length


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()


def _conv(x, w, b):
    """x (B, P, Cin), w (Cout, Cin, k) -> (B, P, Cout), same padding"""
    return F.conv1d(x.transpose(1, 2), w, b, padding=w.shape[2] // 2).transpose(1, 2)


def ffn_ref(x, lens, w1, b1, w2, b2, gamma, beta, eps=1e-5, keep=None, scale=1.0):
    """-> dict(y, h, z1, s, mean, rstd, xhat, xm), fp64, zeros behind the lengths.  keep: None or bool (B, Pmax, D); scale: the
    fp32 value 1 / (1 - p) the kernels multiply by."""
    x, w1, b1, w2, b2, gamma, beta = (_t(v).double() for v in (x, w1, b1, w2, b2, gamma, beta))
    zero = torch.zeros((), dtype=torch.float64)
    valid = valid_mask(lens, x.shape[1])[:, :, None]
    xm = torch.where(valid, x, zero)
    z1 = torch.where(valid, _conv(xm, w1, b1), zero)
    h = torch.relu(z1)
    z = _conv(h, w2, b2)
    if keep is not None:
        z = z * _t(keep).double() * scale
    s = torch.where(valid, xm + z, zero)
    mean = s.mean(-1)
    rstd = 1.0 / torch.sqrt(s.var(-1, unbiased=False) + eps)
    xhat = (s - mean[:, :, None]) * rstd[:, :, None]
    y = xhat * gamma + beta
    v2 = valid[:, :, 0]
    return dict(y=torch.where(valid, y, zero), h=h, z1=z1, s=s, mean=torch.where(v2, mean, zero), rstd=torch.where(v2, rstd, zero),
                xhat=torch.where(valid, xhat, zero), xm=xm)


def _conv_grads(dz, xin, w):
    """dz (B, P, Cout), the convolution's input xin (B, P, Cin), w (Cout, Cin, k) -> (d xin, dw, dbias)"""
    P, k = dz.shape[1], w.shape[2]
    pad = k // 2
    xp, dzp = F.pad(xin, (0, 0, pad, pad)), F.pad(dz, (0, 0, pad, pad))
    dw = torch.stack([torch.einsum("bpo,bpi->oi", dz, xp[:, j:j + P]) for j in range(k)], dim=2)
    dx = sum(torch.einsum("bpo,oi->bpi", dzp[:, 2 * pad - j:2 * pad - j + P], w[:, :, j]) for j in range(k))
    return dx, dw, dz.sum((0, 1))


def ffn_bwd_ref(dy, fwd, lens, w1, w2, gamma, gate, keep=None, scale=1.0):
    """the sublayer's backward from dy (NaN behind the lengths allowed) and `ffn_ref`'s dict; gate: bool (B, Pmax, Chid), where
    the ReLU passes -> dict(dx, dw1, db1, dw2, db2, dgamma, dbeta, ds, dz2, dz1)"""
    dy, w1, w2, gamma, gate = _t(dy).double(), _t(w1).double(), _t(w2).double(), _t(gamma).double(), _t(gate).double()
    zero = torch.zeros((), dtype=torch.float64)
    valid = valid_mask(lens, dy.shape[1])[:, :, None]
    g = torch.where(valid, dy, zero)
    xhat, rstd = fwd["xhat"], fwd["rstd"]
    dgamma, dbeta = (g * xhat).sum((0, 1)), g.sum((0, 1))
    gg = g * gamma
    ds = rstd[:, :, None] * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    dz2 = ds if keep is None else ds * _t(keep).double() * scale
    dh, dw2, db2 = _conv_grads(dz2, fwd["h"], w2)
    dz1 = torch.where(valid, dh * gate, zero)
    dxc, dw1, db1 = _conv_grads(dz1, fwd["xm"], w1)
    dx = torch.where(valid, dxc + ds, zero)
    return dict(dx=dx, dw1=dw1, db1=db1, dw2=dw2, db2=db2, dgamma=dgamma, dbeta=dbeta, ds=ds, dz2=dz2, dz1=dz1)


# ------------------------------------------------------------------------------------------------ block, stack, student
BLOCK_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm.weight",
                "norm.bias", "ffn.w_1.weight", "ffn.w_1.bias", "ffn.w_2.weight", "ffn.w_2.bias", "ffn.layer_norm.weight",
                "ffn.layer_norm.bias")                               # the order of FFTBlock.state_dict()


def _valid(lens, P, device):
    return torch.arange(P, device=device)[None, :] < torch.as_tensor(lens, device=device).clamp(0, P)[:, None]


def _ffn(x, valid, p, pre, eps):
    """the stock chain: where -> Conv1d -> ReLU -> Conv1d -> add -> layer_norm -> where, in x's dtype"""
    zero = x.new_zeros(())
    xm = torch.where(valid, x, zero)
    h = torch.relu(torch.where(valid, _conv(xm, p[pre + "w_1.weight"], p[pre + "w_1.bias"]), zero))
    s = xm + _conv(h, p[pre + "w_2.weight"], p[pre + "w_2.bias"])
    return torch.where(valid, F.layer_norm(s, s.shape[-1:], p[pre + "layer_norm.weight"], p[pre + "layer_norm.bias"], eps), zero)


def fft_block_ref(x, lens, p, n_head, pre="", eps=1e-5):
    """FFTBlock in stock torch, dropout off: `nn.MultiheadAttention`'s functional form under a key-padding mask, residual,
    LayerNorm, then the conv feed-forward; p: name -> tensor (BLOCK_PARAMS behind `pre`); differentiable; x's dtype and device.
    Every length must be at least 1 (a row of the softmax with no key has no value in torch)."""
    B, P, D = x.shape
    valid = _valid(lens, P, x.device)
    a, _ = F.multi_head_attention_forward(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), D, n_head, p[pre + "self_attn.in_proj_weight"],
                                          p[pre + "self_attn.in_proj_bias"], None, None, False, 0.0, p[pre + "self_attn.out_proj.weight"],
                                          p[pre + "self_attn.out_proj.bias"], training=False, key_padding_mask=~valid, need_weights=False)
    s = F.layer_norm(x + a.transpose(0, 1), (D,), p[pre + "norm.weight"], p[pre + "norm.bias"], eps)
    return _ffn(s, valid[:, :, None], p, pre + "ffn.", eps)


def sinusoids(n, d, dtype=torch.float64):
    pos = torch.arange(n, dtype=torch.float64)[:, None]
    inv = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * (-math.log(10000.0) / d))
    pe = torch.zeros(n, d, dtype=torch.float64)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * inv), torch.cos(pos * inv)
    return pe.to(torch.float32).to(dtype)                            # (the module's table is the fp32 rounding of these)


def fft_stack_ref(x, lens, p, n_layers, n_head, pre="", eps=1e-5):
    B, P, D = x.shape
    valid = _valid(lens, P, x.device)[:, :, None]
    x = torch.where(valid, x + sinusoids(P, D, x.dtype).to(x.device), x.new_zeros(()))
    for i in range(n_layers):
        x = fft_block_ref(x, lens, p, n_head, f"{pre}layers.{i}.", eps)
    return x


def _predictor(x, valid, p, pre, eps):
    zero = x.new_zeros(())
    h = x
    for i in ("1", "2"):
        h = torch.relu(_conv(torch.where(valid, h, zero), p[pre + f"conv{i}.weight"], p[pre + f"conv{i}.bias"]))
        h = F.layer_norm(h, h.shape[-1:], p[pre + f"norm{i}.weight"], p[pre + f"norm{i}.bias"], eps)
    out = F.linear(h, p[pre + "out.weight"], p[pre + "out.bias"])[:, :, 0]
    return torch.where(valid[:, :, 0], out, zero)


def student_ref(p, cfg, phoneme, lens, durations, pitch, energy, Tmax, eps=1e-5):
    """FastSpeech2Student's training forward (targets given, dropout off) in stock torch; p: the module's `state_dict` in the
    wanted dtype plus the buffers 'adaptor.embedding.pitch_bins' / 'energy_bins' (fp32 boundaries, compared in fp32 as the kernel
    does); cfg: dict(encoder_layers, decoder_layers, n_head); durations int64, zero or more frames per valid phoneme
    -> dict(melspec, log_duration, pitch, energy, mel_lens)"""
    dev = p["embedding.weight"].device
    B, P = phoneme.shape
    valid = _valid(lens, P, dev)
    x = fft_stack_ref(F.embedding(phoneme, p["embedding.weight"]), lens, p, cfg["encoder_layers"], cfg["n_head"], "encoder.", eps)
    v3 = valid[:, :, None]
    out = {k: _predictor(x, v3, p, f"adaptor.{n}_predictor.", eps) for k, n in (("log_duration", "duration"), ("pitch", "pitch"), ("energy", "energy"))}
    ip = torch.bucketize(pitch.float(), p["adaptor.embedding.pitch_bins"].float())
    ie = torch.bucketize(energy.float(), p["adaptor.embedding.energy_bins"].float())
    h = torch.where(v3, (x + p["adaptor.embedding.pitch_table"][ip]) + p["adaptor.embedding.energy_table"][ie], x)
    dur = torch.where(valid, durations.clamp(min=0), torch.zeros_like(durations))
    mel_lens = dur.sum(1).clamp(max=Tmax)
    frames = x.new_zeros(B, Tmax, x.shape[2])
    for b in range(B):
        rows = torch.repeat_interleave(h[b], dur[b], dim=0)[:Tmax]
        frames[b, :rows.shape[0]] = rows
    y = fft_stack_ref(frames, mel_lens, p, cfg["decoder_layers"], cfg["n_head"], "decoder.", eps)
    mel = F.linear(y, p["mel_linear.weight"], p["mel_linear.bias"])
    out["melspec"] = torch.where(_valid(mel_lens, Tmax, dev)[:, :, None], mel, mel.new_zeros(()))
    out["mel_lens"] = mel_lens
    return out
