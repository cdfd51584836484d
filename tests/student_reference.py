"""fp64 restatement of the student's mel loss (csrc/student_loss.hip) as an explicit mask over n_b = min(pred_lens[b],
target_lens[b]) clipped to [0, min(T, Tt)], its closed-form gradient, and the fixtures the host and the device tests share: fp32
operands whose differences stay away from the kink of |d| (|d| >= MIN_DIFF), with NaN at and behind every n_b of BOTH operands.
tests/test_student_host.py holds the restatement to torch.nn.functional.l1_loss / mse_loss on the selected elements and its
gradient to autograd."""
import functools

import numpy as np
import torch

MIN_DIFF = 1e-3


def frames_ref(pred_lens, target_lens, T, Tt):
    """n_b as a list of Python ints"""
    hi = min(int(T), int(Tt))
    return [max(0, min(int(a), int(b), hi)) for a, b in zip(pred_lens, target_lens)]


def mel_mask(pred_lens, target_lens, T, Tt, rows):
    """bool (B, rows, 1): frame t of utterance b counts"""
    n = torch.tensor(frames_ref(pred_lens, target_lens, T, Tt))
    return (torch.arange(rows)[None, :] < n[:, None])[:, :, None]


def _f64(a):
    """fp64 on the host; a tensor keeps its place in the autograd graph"""
    return (a.cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).double()


def mel_loss_ref(pred, pred_lens, target, target_lens, weights=(1.0, 0.0), extra=None):
    """-> dict(mae, mse, mel, total: 0-dim fp64; frames: int), every term exactly 0 when frames is 0.  Elements at or behind n_b
    are never touched (a NaN there does not matter): the sums run over explicit slices."""
    pred, target = _f64(pred), _f64(target)
    B, T, M = pred.shape
    n = frames_ref(pred_lens, target_lens, T, target.shape[1])
    N = sum(n)
    s_abs = s_sq = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        d = pred[b, :n[b]] - target[b, :n[b]]
        s_abs = s_abs + d.abs().sum()
        s_sq = s_sq + (d * d).sum()
    mae, mse = (s_abs / (N * M), s_sq / (N * M)) if N > 0 else (s_abs * 0, s_sq * 0)
    mel = weights[0] * mae + weights[1] * mse
    total = mel if extra is None else mel + (_f64(extra).reshape(()) if isinstance(extra, torch.Tensor) else float(extra))
    return {"mae": mae, "mse": mse, "mel": mel, "total": total, "frames": N}


def mel_loss_grad_ref(pred, pred_lens, target, target_lens, weights=(1.0, 0.0), g=(0.0, 0.0, 0.0, 1.0)):
    """d(sum_k g_k out_k) / d pred in closed form, g = (g_mae, g_mse, g_mel, g_total): ((g_total + g_mel) w_mae + g_mae) sign(d) /
    (N M) + ((g_total + g_mel) w_mse + g_mse) 2 d / (N M) for t < n_b, exact zeros elsewhere (and everywhere when N = 0);
    sign(0) = 0, as torch's abs backward gives.  (B, T, M) fp64."""
    pred, target = _f64(pred).detach(), _f64(target).detach()
    B, T, M = pred.shape
    n = frames_ref(pred_lens, target_lens, T, target.shape[1])
    N = sum(n)
    out = torch.zeros(B, T, M, dtype=torch.float64)
    if N == 0:
        return out
    up = float(g[3]) + float(g[2])
    c_abs, c_sq = up * weights[0] + float(g[0]), up * weights[1] + float(g[1])
    for b in range(B):
        d = pred[b, :n[b]] - target[b, :n[b]]
        out[b, :n[b]] = c_abs * torch.sign(d) / (N * M) + c_sq * 2.0 * d / (N * M)
    return out


def mel_loss_stock(pred, pred_lens, target, target_lens, weights=(1.0, 0.0), extra=None):
    """the `where` / `abs` / `sum` / `div` restatement a user would write, in pred's dtype and on its device; differentiable"""
    B, T, M = pred.shape
    Tt = target.shape[1]
    rows = min(T, Tt)
    dev = pred.device
    n = torch.minimum(torch.as_tensor(pred_lens, device=dev), torch.as_tensor(target_lens, device=dev)).clamp(0, rows)
    keep = (torch.arange(rows, device=dev)[None, :] < n[:, None])[:, :, None]
    zero = pred.new_zeros(())
    d = torch.where(keep, pred[:, :rows] - target[:, :rows].to(pred.dtype), zero)
    den = (n.sum() * M).to(pred.dtype).clamp(min=1)
    mae, mse = d.abs().sum() / den, (d * d).sum() / den
    mel = weights[0] * mae + weights[1] * mse
    return {"mae": mae, "mse": mse, "mel": mel, "total": mel if extra is None else mel + extra, "frames": n.sum()}


@functools.lru_cache(maxsize=None)
def mel_case(B, T, Tt, M, pred_lens, target_lens, seed=0, zeros=False):
    """-> dict(pred (B, T, M), target (B, Tt, M): fp32 numpy with NaN at and behind every n_b of both; pred_lens, target_lens:
    int64 numpy; n: list).  |pred - target| >= MIN_DIFF on every counted element -- except, with zeros=True, a planted quarter
    where pred == target bit for bit ('planted': bool (B, T, M)).  Made once per argument set; never written to."""
    rng = np.random.default_rng(1000 + seed + 7 * B + 11 * T + 13 * Tt + 17 * M)
    pred = rng.standard_normal((B, T, M)).astype(np.float32)
    target = rng.standard_normal((B, Tt, M)).astype(np.float32)
    rows = min(T, Tt)
    d = pred[:, :rows] - target[:, :rows]
    near = np.abs(d) < 2 * MIN_DIFF
    pred[:, :rows][near] += np.float32(0.25)
    planted = np.zeros((B, T, M), dtype=bool)
    if zeros:
        planted[:, :rows] = rng.random((B, rows, M)) < 0.25
        pred[:, :rows][planted[:, :rows]] = target[:, :rows][planted[:, :rows]]
    n = frames_ref(pred_lens, target_lens, T, Tt)
    for b in range(B):
        pred[b, n[b]:] = np.nan
        target[b, n[b]:] = np.nan
        planted[b, n[b]:] = False
    return dict(pred=pred, target=target, pred_lens=np.array(pred_lens, np.int64), target_lens=np.array(target_lens, np.int64), n=n,
                planted=planted)


def counted_diffs(case):
    """the fp32 differences of the counted elements, flat"""
    return np.concatenate([(case["pred"][b, :k] - case["target"][b, :k]).reshape(-1) for b, k in enumerate(case["n"])] or [np.zeros(0)])
