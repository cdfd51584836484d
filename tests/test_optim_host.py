"""The fp64 oracles behind tests/test_hip_optim.py, held to what they restate: tests/optim_reference.py against the real
torch.optim.Adam + torch.nn.utils.clip_grad_norm_ in fp64 (several tensors of unequal shapes, clipped and unclipped steps in
turn), oracle.noam_lambda against utils.util.get_noam_scheduler around the warm-up, and oracle_loss with an EMPTY utterance beside
non-empty ones against the loss of the batch without it.  Host arithmetic only, no GPU."""
import math

import torch

from optim_reference import BETAS, BOUND, EPS, FACTOR, SIZES, STOCK_WORST, clip_adam_step, grad_norm, rel, stock_step


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def test_flat_fp64_step_is_torch_adam_behind_clip_grad_norm():
    """Six steps over five tensors: the flat restatement (one concatenated buffer) and torch's per-tensor optimizer agree to 1e-12
    relative in the update, the parameters, both moments and the clip coefficient; steps 1, 3, 5 clip (norm >> 1), 2, 4, 6 do not."""
    shapes = [(37, 64), (130,), (5, 3, 7), (1,), (33, 9)]
    sizes = [math.prod(s) for s in shapes]
    ps = [torch.nn.Parameter(_rand(*s, seed=10 + i, scale=0.05)) for i, s in enumerate(shapes)]
    opt = torch.optim.Adam(ps, lr=1e-3, betas=BETAS, eps=EPS)
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])      # noqa: E731
    p = flat(ps).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    clipped = []
    for step in range(1, 7):
        lr = 1e-3 * (0.5 + 0.25 * step)                      # (a rate that moves, as under a schedule)
        for i, (q, s) in enumerate(zip(ps, shapes)):
            q.grad = _rand(*s, seed=100 * step + i, scale=3.0 if step % 2 else 1e-4)
        g = flat([q.grad for q in ps]).clone()
        assert abs(grad_norm(g) - float(torch.linalg.vector_norm(g))) <= 1e-12 * grad_norm(g)
        total = torch.nn.utils.clip_grad_norm_(ps, 1.0)
        assert abs(float(total) - grad_norm(g)) <= 1e-12 * grad_norm(g)
        opt.param_groups[0]["lr"] = lr
        before = flat(ps).clone()
        opt.step()
        p_new, m, v, coef = clip_adam_step(p, g, m, v, step, lr, BETAS, EPS, 1.0)
        clipped.append(coef < 1.0)
        want_coef = min(1.0, 1.0 / (float(total) + 1e-6))
        assert abs(coef - want_coef) <= 1e-12 * want_coef
        assert rel(flat([q.grad for q in ps]), g * coef) < 1e-12                     # what clip_grad_norm_ left in .grad
        assert rel(p_new - p, flat(ps) - before) < 1e-12, step                       # the update
        assert rel(p_new, flat(ps)) < 1e-12
        assert rel(m, flat([opt.state[q]["exp_avg"] for q in ps])) < 1e-12, step
        assert rel(v, flat([opt.state[q]["exp_avg_sq"] for q in ps])) < 1e-12, step
        assert int(opt.state[ps[0]]["step"]) == step
        p = p_new
    assert clipped == [True, False, True, False, True, False]
    assert sum(sizes) == p.numel()


def test_flat_fp64_step_without_clipping_and_from_given_moments():
    """max_norm None and 0 both mean no clipping (torch: no clip_grad_norm_ call); a step in the middle of a run (step 1000,
    non-zero moments) against torch.optim.Adam with that state; the inputs are not written to."""
    n = 1000
    p, g = _rand(n, seed=1, scale=0.05), _rand(n, seed=2, scale=3.0)
    m, v = _rand(n, seed=3, scale=0.01), _rand(n, seed=4, scale=0.01) ** 2
    keep = [t.clone() for t in (p, g, m, v)]
    for max_norm in (None, 0.0, 1.0):
        for step, mm, vv in ((1, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)), (1000, m, v)):
            got = clip_adam_step(p, g, mm, vv, step, 1e-3, BETAS, EPS, max_norm)
            want = stock_step(p, g, mm, vv, step, 1e-3, BETAS, EPS, max_norm, dtype=torch.float64)
            assert (got[3] == 1.0) == (not max_norm)
            assert rel(got[0] - p, want[0] - p) < 1e-12 and rel(got[1], want[1]) < 1e-12 and rel(got[2], want[2]) < 1e-12
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, g, m, v)))


def test_the_bounds_follow_from_the_stock_figures():
    assert FACTOR == 4.0 and set(BOUND) == set(STOCK_WORST) == {"update", "exp_avg", "exp_avg_sq"}
    assert all(BOUND[k] == 4.0 * STOCK_WORST[k] for k in BOUND)
    # far below what a wrong optimizer shows against the same fp64 step (no clipping: update 2.1e-2, exp_avg 0.64; bias correction
    # one step late: update 0.26; beta2 0.999: exp_avg_sq 0.95)
    assert BOUND["update"] < 2.1e-2 / 100 and BOUND["exp_avg"] < 0.64 / 100 and BOUND["exp_avg_sq"] < 0.95 / 100
    # the sizes: float4s per buffer against the caps of the two grids (1024 and 2048 blocks of 256 threads)
    assert [n // 4 for n in SIZES] == [1, 256, 257, 1024 * 256 + 1, 2048 * 256 + 1, 2 * 2048 * 256 + 777]
    assert all(n % 4 == 0 for n in SIZES)


def test_noam_lambda_is_the_shipped_schedule_around_the_warm_up():
    from oracle.ref_model import noam_lambda
    from transformertts_amd.utils.util import get_noam_scheduler
    for d_model, warm in ((256, 4000), (64, 50)):
        ref, got = noam_lambda(d_model, warm), get_noam_scheduler(d_model, warm)
        for s in (0, 1, 2, warm - 1, warm, warm + 1):
            assert abs(got(s) - ref(s)) <= 1e-15 * ref(s), (d_model, warm, s)
        assert ref(0) == ref(1) and ref(warm) > ref(warm - 1) and ref(warm) > ref(warm + 1)        # the peak is at the warm-up
        assert abs(ref(warm) - (d_model * warm) ** -0.5) <= 1e-15


def test_oracle_loss_takes_an_empty_utterance():
    """Lengths [T, 1, 0, 7]: the empty utterance adds nothing to any of the four losses -- they equal the losses of the batch
    without it -- and gets all-zero gradients; nothing is NaN."""
    from oracle import oracle_loss
    B, T, C = 4, 37, 16
    lens = torch.tensor([T, 1, 0, 7])
    pred, post, stop, mel = (_rand(B, T, C, seed=1), _rand(B, T, C, seed=2), _rand(B, T, seed=3, scale=2.0), _rand(B, T, C, seed=4))
    pd, qd, sd = [t.clone().requires_grad_() for t in (pred, post, stop)]
    full = oracle_loss({"pred_melspec": pd, "post_melspec": qd, "pred_stop": sd}, mel, lens)
    full["total"].backward()
    keep = torch.tensor([0, 1, 3])
    part = oracle_loss({"pred_melspec": pred[keep], "post_melspec": post[keep], "pred_stop": stop[keep]}, mel[keep], lens[keep])
    for k in ("total", "pred_mel", "post_mel", "stop"):
        assert torch.isfinite(full[k]) and abs(float(full[k].detach()) - float(part[k])) <= 1e-13 * abs(float(part[k])), k
    for gr in (pd.grad, qd.grad, sd.grad):
        assert torch.isfinite(gr).all() and float(gr[2].abs().max()) == 0.0 and float(gr[0].abs().max()) > 0.0
    # by the definition: mean over valid frames x channels, stop target 1 at the last valid frame, weight 8 there
    valid = torch.arange(T)[None, :] < lens[:, None]
    n = int(valid.sum())
    assert n == T + 1 + 7
    want_pred = float((((pred - mel) ** 2) * valid[..., None]).sum() / (n * C))
    gate = (torch.arange(T)[None, :] == (lens[:, None] - 1)).double()
    bce = (1 - gate) * stop + (1 + 7.0 * gate) * torch.nn.functional.softplus(-stop)
    want_stop = float((bce * valid).sum() / n)
    assert abs(float(full["pred_mel"].detach()) - want_pred) <= 1e-13 * want_pred
    assert abs(float(full["stop"].detach()) - want_stop) <= 1e-13 * want_stop
