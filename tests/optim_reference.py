"""fp64 restatement of what one optimizer step of the training loop computes over FLAT tensors -- global-norm clipping as
torch.nn.utils.clip_grad_norm_ does it (coef = min(1, max_norm / (norm + 1e-6))) followed by torch.optim.Adam (no amsgrad, no
weight decay, betas as Python doubles) -- plus the stock fp32 form of the same step, which is the yardstick the kernels'
bounds come from.  tests/test_optim_host.py holds the restatement to the real torch.optim.Adam + clip_grad_norm_ in fp64.

What is measured, everywhere this file is used: the UPDATE p_after - p_before (subtracted in fp64) and both moments, each as a
relative L2 error against the fp64 step.  Never the parameter: at the Noam rate an update is 1e-6 of the parameter or less, so a
parameter-relative error cannot tell an optimizer that does nothing from a correct one.

Bounds.  STOCK_WORST is the worst error, per measure, of the stock fp32 form (torch.optim.Adam + clip_grad_norm_ on fp32 CPU
tensors) against the fp64 step over every case of tests/test_hip_optim.py -- sizes 4 .. 4 197 412, lr 1e-3, parameters of scale
0.05, clipped and unclipped gradients, steps 1, 2, 3 and 1000 (measured on the CPU; tests/reports/optim_margin.txt lists the
stock figure of every case beside the kernel's).  All three worst figures come from clipped steps at n = 4 197 412, where the stock
form's fp32 norm of four million elements is 1e-4 off and the coefficient with it; below a million elements and without clipping
the stock form stays under 2.5e-6 / 1e-7 / 1.5e-7, and the kernels measure 2.2e-6 / 2.9e-7 / 1.1e-6 at every size (their 1.f - beta2
in fp32 is 9.5e-7 off 0.02).  A kernel is held to BOUND = 4 x STOCK_WORST: the factor allows for the different
summation order of the norm and for 1.f - beta being taken in fp32 in the kernel."""
import math

import torch

BETAS, EPS, LR = (0.9, 0.98), 1e-9, 1e-3      # the reference's Adam; LR: the shipped peak 256^-0.5 * 4000^-0.5 = 9.9e-4, rounded
P_SCALE = 0.05
FACTOR = 4.0
STOCK_WORST = {"update": 2.97e-5, "exp_avg": 9.50e-5, "exp_avg_sq": 1.90e-4}
BOUND = {k: FACTOR * v for k, v in STOCK_WORST.items()}


def grad_norm(g) -> float:
    """|| g ||_2 of a flat tensor, in fp64"""
    return float(g.detach().double().cpu().reshape(-1).norm())


def clip_adam_step(p, g, m, v, step, lr, betas=BETAS, eps=EPS, max_norm=None):
    """One step on flat tensors, in fp64 -> (p, m, v, coef); the inputs are left as they were.  `max_norm` None or <= 0: no
    clipping (coef 1)."""
    p, g, m, v = (t.detach().double().cpu().reshape(-1) for t in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    coef = 1.0
    if max_norm is not None and max_norm > 0:
        coef = min(1.0, float(max_norm) / (grad_norm(g) + 1e-6))
    g = g * coef
    m = m + (g - m) * (1.0 - b1)                                    # exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + g * g * (1.0 - b2)                                 # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (float(lr) / bc1) * (m / denom)
    return p, m, v, coef


def stock_step(p, g, m, v, step, lr, betas=BETAS, eps=EPS, max_norm=None, dtype=torch.float32):
    """The same step by torch.optim.Adam + torch.nn.utils.clip_grad_norm_ themselves on CPU tensors of `dtype` -> (p, m, v)"""
    q = torch.nn.Parameter(p.detach().cpu().to(dtype).reshape(-1).clone())
    q.grad = g.detach().cpu().to(dtype).reshape(-1).clone()
    opt = torch.optim.Adam([q], lr=float(lr), betas=betas, eps=eps)
    if step > 1 or bool(m.any()) or bool(v.any()):
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().cpu().to(dtype).reshape(-1).clone(),
                        "exp_avg_sq": v.detach().cpu().to(dtype).reshape(-1).clone()}
    if max_norm is not None and max_norm > 0:
        torch.nn.utils.clip_grad_norm_([q], float(max_norm))
    opt.step()
    st = opt.state[q]
    assert int(st["step"]) == step
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def rel(a, b) -> float:
    """|| a - b || / || b || in fp64 (|| a - b || where b is all zero)"""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


# ---- the cases of tests/test_hip_optim.py (inputs only; made once per size and never written to)
# n -> the branch it covers.  Both kernels run blocks of 256 threads, one float4 per thread and sweep, so a block covers 1024
# floats; ttts_grad_norm caps its grid at 1024 blocks (one sweep: 1 048 576 floats), ttts_adam_step at 2048 (2 097 152 floats).
SIZES = {4: "one float4 (grids 1 / 1)",
         1024: "exactly one block (grids 1 / 1)",
         1028: "one block plus one lane (grids 2 / 2)",
         1048580: "n4 = 262 145: the sum of squares runs 1024 blocks and wraps by one float4 (Adam: 1025 blocks, one sweep)",
         2097156: "n4 = 524 289: Adam runs 2048 blocks and wraps by one float4 (sum of squares: two sweeps plus one)",
         4197412: "n4 = 1 049 353 = 2 x 524 288 + 777: two full sweeps of the Adam grid and a ragged third (777 float4s: 3 blocks "
                  "and 9 lanes)"}
_CACHE = {}


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def case_inputs(n):
    """-> dict: p (scale 0.05), g_big / g_big2 (global norm 3 sqrt(n) >> 1: clipped), g_small (global norm 0.01 << 1: not
    clipped), and plausible moments m1, v1 of a run in progress (for steps past the first)"""
    if n not in _CACHE:
        g_run = _randn(n, 7) / math.sqrt(n)                         # a clipped gradient: global norm 1
        _CACHE[n] = {"p": _randn(n, 1) * P_SCALE, "g_big": _randn(n, 2) * 3.0, "g_small": _randn(n, 3) * (0.01 / math.sqrt(n)),
                     "g_big2": _randn(n, 4) * 3.0, "m1": (_randn(n, 5) / math.sqrt(n) + g_run) * 0.5,
                     "v1": (_randn(n, 6) / math.sqrt(n)) ** 2 * 0.5 + g_run * g_run * 0.5}
    return _CACHE[n]


def case_list(n):
    """-> [(label, start moments or None for zeros, [(gradient key, step, how), ...])]: runs of consecutive steps that carry the
    moments.  `how`: "clip" (max norm 1), "null" (clip disabled by a NULL norm pointer), "max0" (disabled by max_grad_norm = 0)."""
    return [("three steps 1-3, clipped / not / clipped", None, [("g_big", 1, "clip"), ("g_small", 2, "clip"), ("g_big2", 3, "clip")]),
            ("clip off: norm pointer NULL", None, [("g_big", 1, "null")]),
            ("clip off: max_grad_norm 0", None, [("g_big", 1, "max0")]),
            ("step 1, not clipped", None, [("g_small", 1, "clip")]),
            ("step 2, clipped", ("m1", "v1"), [("g_big2", 2, "clip")]),
            ("step 1000, clipped", ("m1", "v1"), [("g_big", 1000, "clip")])]


def run_case(n, start, steps, step_fn):
    """Run `steps` from the case inputs of size n; `step_fn(p, g, m, v, step, how) -> (p, m, v)` is the form under test (it gets
    its own form's previous results), the fp64 step runs beside it from ITS own previous results.  -> [(errors of the step,
    clip coefficient the fp64 step used)]"""
    c = case_inputs(n)
    zeros = torch.zeros(n)
    p, m, v = c["p"], (c[start[0]] if start else zeros), (c[start[1]] if start else zeros)
    rp, rm, rv = p, m, v
    out = []
    for key, step, how in steps:
        p0, r0 = p, rp
        p, m, v = step_fn(p, c[key], m, v, step, how)
        rp, rm, rv, coef = clip_adam_step(rp, c[key], rm, rv, step, LR, max_norm=1.0 if how == "clip" else None)
        # each side's update is taken from its own previous parameters (which differ by fp32 rounding after the first step)
        e = {"update": rel(p.double().cpu() - p0.double().cpu(), rp - r0.double()), "exp_avg": rel(m, rm), "exp_avg_sq": rel(v, rv)}
        out.append((e, coef))
    return out


def stock_fn(p, g, m, v, step, how):
    return stock_step(p, g, m, v, step, LR, max_norm=1.0 if how == "clip" else None)
