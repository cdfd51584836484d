"""fp64 oracles of the ragged Conv1d -> ReLU -> LayerNorm -> Dropout stage and of the variance predictor built from it
(csrc/predictor.hip, transformertts_amd/predictor.py), written from the definition in DESIGN.md 27.  torch fp64 on the CPU; the
forward is differentiable (autograd gives the predictor's gradients), and `stage_bwd_ref` restates the backward formula by formula
with the ReLU gate as an INPUT, so a test can hand it the gate a kernel took.  Test infrastructure, no GPU."""
import numpy as np
import torch
from torch.nn import functional as F


def valid_mask(lens, Pmax):
    lens = torch.as_tensor(np.asarray(lens)).clamp(0, Pmax)
    return torch.arange(Pmax)[None, :] < lens[:, None]


def poison(lens, *arrays):
    """copies of (B, Pmax, ...) arrays with NaN at and behind every length"""
    out = []
    for a in arrays:
        a = np.array(a, copy=True)
        for b, n in enumerate(lens):
            a[b, max(int(n), 0):] = np.nan
        out.append(a)
    return out[0] if len(out) == 1 else out


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()


def stage_ref(x, lens, w, bias, gamma, beta, eps=1e-5, keep=None, scale=1.0):
    """-> dict(y, r, mean, rstd, z, xhat, xm), all fp64, zeros behind the lengths (z too).  keep: None or bool (B, Pmax, Cout);
    scale: the fp32 value 1 / (1 - p) the kernels multiply by."""
    x, w, bias, gamma, beta = (_t(v).double() for v in (x, w, bias, gamma, beta))
    B, Pmax, _ = x.shape
    k = w.shape[2]
    valid = valid_mask(lens, Pmax)[:, :, None]
    xm = torch.where(valid, x, torch.zeros((), dtype=torch.float64))
    z = F.conv1d(xm.transpose(1, 2), w, bias, padding=k // 2).transpose(1, 2)
    r = torch.relu(z)
    mean = r.mean(-1)
    rstd = 1.0 / torch.sqrt(r.var(-1, unbiased=False) + eps)
    xhat = (r - mean[:, :, None]) * rstd[:, :, None]
    y = xhat * gamma + beta
    if keep is not None:
        y = y * _t(keep).double() * scale
    zero = torch.zeros((), dtype=torch.float64)
    v2 = valid[:, :, 0]
    return dict(y=torch.where(valid, y, zero), r=torch.where(valid, r, zero), mean=torch.where(v2, mean, zero),
                rstd=torch.where(v2, rstd, zero), z=torch.where(valid, z, zero), xhat=torch.where(valid, xhat, zero), xm=xm)


def stage_bwd_ref(dy, fwd, lens, w, gamma, gate, keep=None, scale=1.0):
    """the stage's backward from dy (NaN behind the lengths allowed) and the forward's dict; gate: bool (B, Pmax, Cout), where
    the ReLU passes -> dict(dx, dw, dbias, dgamma, dbeta, dz)"""
    dy, w, gamma, gate = _t(dy).double(), _t(w).double(), _t(gamma).double(), _t(gate).double()
    B, Pmax, Cout = dy.shape
    k = w.shape[2]
    pad = k // 2
    valid = valid_mask(lens, Pmax)[:, :, None]
    g = torch.where(valid, dy, torch.zeros((), dtype=torch.float64))
    if keep is not None:
        g = g * _t(keep).double() * scale
    xhat, rstd, xm = fwd["xhat"], fwd["rstd"], fwd["xm"]
    dgamma, dbeta = (g * xhat).sum((0, 1)), g.sum((0, 1))
    gg = g * gamma
    dr = rstd[:, :, None] * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    dz = dr * gate
    xp, dzp = F.pad(xm, (0, 0, pad, pad)), F.pad(dz, (0, 0, pad, pad))
    dw = torch.stack([torch.einsum("bpo,bpi->oi", dz, xp[:, j:j + Pmax]) for j in range(k)], dim=2)
    dx = sum(torch.einsum("bpo,oi->bpi", dzp[:, 2 * pad - j:2 * pad - j + Pmax], w[:, :, j]) for j in range(k))
    dx = torch.where(valid, dx, torch.zeros((), dtype=torch.float64))
    return dict(dx=dx, dw=dw, dbias=dz.sum((0, 1)), dgamma=dgamma, dbeta=dbeta, dz=dz)


PARAMS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias",
          "out.weight", "out.bias")                                   # the order of VariancePredictor.state_dict()


def predictor_ref(x, lens, params, eps=1e-5):
    """stage -> stage -> head in fp64 (eval: no dropout); params: name -> array, the names of PARAMS -> (B, Pmax), zeros behind"""
    p = {k: _t(v).double() for k, v in params.items()}
    h = stage_ref(x, lens, p["conv1.weight"], p["conv1.bias"], p["norm1.weight"], p["norm1.bias"], eps)["y"]
    h = stage_ref(h, lens, p["conv2.weight"], p["conv2.bias"], p["norm2.weight"], p["norm2.bias"], eps)["y"]
    out = h @ p["out.weight"][0] + p["out.bias"][0]
    return torch.where(valid_mask(lens, h.shape[1]), out, torch.zeros((), dtype=torch.float64))


def predictor_grads_ref(x, lens, params, dout, eps=1e-5):
    """-> out, dx, {name: gradient}: autograd through `predictor_ref` (dout may hold NaN behind the lengths: not used)"""
    x = torch.where(valid_mask(lens, x.shape[1])[:, :, None], _t(x).double(), torch.zeros((), dtype=torch.float64)).requires_grad_(True)
    p = {k: _t(v).double().clone().requires_grad_(True) for k, v in params.items()}
    out = predictor_ref(x, lens, p, eps)
    g = torch.where(valid_mask(lens, x.shape[1]), _t(dout).double(), torch.zeros((), dtype=torch.float64))
    grads = torch.autograd.grad(out, [x] + [p[k] for k in PARAMS], g)
    return out.detach(), grads[0], dict(zip(PARAMS, grads[1:]))
