"""The two ends of every training step against fp64: csrc/optim.hip (ttts_grad_norm, ttts_adam_step, the per-step state block)
and, under "step head", csrc/loss.hip (loss forward / backward, the scheduled-sampling mix) at the sizes where their capped
grid-stride loops wrap, which is how the shipped step runs all of them.

Optimizer measure: the UPDATE p_after - p_before (subtracted in fp64) and both moments, each relative-L2 against the fp64 step of
tests/optim_reference.py, at lr 1e-3 (the shipped peak rate) on parameters of scale 0.05 -- an update is then 1e-3 per element,
far above the fp32 rounding of the parameter, and a wrong clip coefficient, moment, bias correction or eps shows at 1e-2 .. 1.
Bound: optim_reference.BOUND = 4 x the worst error of the stock fp32 form (torch.optim.Adam + clip_grad_norm_ on the CPU) on that
measure.  Every launch is made twice and must give the same bits.  Measured figures, stock beside kernel:
parity_reports/optim_margin.txt (as measured on one MI355X: tests/reports/optim_margin.txt).

Grids (derived from the sources; the library has no query for them).  Both optimizer kernels run 256 threads a block and one
float4 per thread and sweep, so a block covers 1024 floats; sumsq_partial_kernel runs min(1024, ceil(n4 / 256)) blocks,
adam_step_kernel min(2048, ceil(n4 / 256)).  optim_reference.SIZES names the branch of each n.  The loss kernels run one float4
of the (B, T, C) tensors per thread and sweep: loss_partial_kernel at most 1024 blocks (262 144 float4s a sweep), loss_bwd_kernel
and sched_mix_kernel at most 2048 (524 288)."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from optim_reference import BETAS, BOUND, EPS, LR, SIZES, case_inputs, case_list, clip_adam_step, grad_norm, rel, run_case, stock_fn
from test_hip_dropout_parity import REPORT_DIR
from test_hip_ops import TOL, _dev, _g, _rand

pytestmark = pytest.mark.gpu
MEASURES = ("update", "exp_avg", "exp_avg_sq")


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/optim_margin.txt", "a") as f:
        f.write(line + "\n")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _norm_once(g):
    from transformertts_amd import _lib, ops
    from transformertts_amd.ops import _p, _stream
    lib = _lib.load()
    norm = torch.full((1,), float("nan"), device=g.device)
    ws = ops._ws(lib.ttts_grad_norm_workspace_bytes(), g.device)
    assert lib.ttts_grad_norm(_p(g), _p(norm), _p(ws), ws.numel() * 4, g.numel(), _stream()) == 0, _lib.last_error()
    return norm


def _adam_once(p, g, m, v, step, how, lr=LR, st=None):
    """ttts_grad_norm (unless the clip is off by a NULL norm pointer) + ttts_adam_step on clones -> (p, m, v, norm or None)"""
    from transformertts_amd import _lib
    from transformertts_amd.ops import _p, _stream
    lib, dev = _lib.load(), _dev()
    p, m, v = (t.to(dev).clone() for t in (p, m, v))
    g = g.to(dev)
    norm = None if how == "null" else _norm_once(g)
    assert lib.ttts_adam_step(_p(p), _p(g), _p(m), _p(v), _p(norm), p.numel(), float(lr), BETAS[0], BETAS[1], EPS, int(step),
                              0.0 if how == "max0" else 1.0, st, _stream()) == 0, _lib.last_error()
    return p, m, v, norm


def _adam_twice(p, g, m, v, step, how, lr=LR, st=None):
    """the launch pair twice from the same inputs: the same bits; -> (p, m, v) on the device"""
    a, b = _adam_once(p, g, m, v, step, how, lr, st), _adam_once(p, g, m, v, step, how, lr, st)
    for x, y in zip(a, b):
        assert (x is None and y is None) or _same_bits(x, y)
    return a[:3]


def _kernel_fn(p, g, m, v, step, how):
    return _adam_twice(p, g, m, v, step, how)


# ------------------------------------------------------------------------------------------------------------ the kernels directly
@pytest.mark.parametrize("n", list(SIZES))
def test_clip_and_adam_kernels_against_fp64(n):
    """Every case of optim_reference.case_list: three consecutive steps carrying the moments with clipped and unclipped gradients
    in turn, the clip disabled by a NULL norm pointer and by max_grad_norm = 0 (on a gradient that WOULD clip), steps 1, 2 and 1000
    -- update and moments under BOUND, the stock fp32 form's figures beside them in the report."""
    _report(f"n {n}: {SIZES[n]}")
    for label, start, steps in case_list(n):
        got, stock = run_case(n, start, steps, _kernel_fn), run_case(n, start, steps, stock_fn)
        for (key, step, how), (e, coef), (s, _) in zip(steps, got, stock):
            _report(f"  {label}: step {step} {key} coef {coef:.3e}: " +
                    " ".join(f"{k} stock {s[k]:.3e} kernel {e[k]:.3e} bound {BOUND[k]:.3e}" for k in MEASURES))
            assert (coef < 1.0) == (how == "clip" and key != "g_small"), (label, step)      # by the fp64 reference alone
            for k in MEASURES:
                assert e[k] < BOUND[k], (n, label, step, k, e[k])


@pytest.mark.parametrize("n", list(SIZES))
def test_grad_norm_kernel_against_fp64(n):
    """ttts_grad_norm alone: |norm - fp64| / fp64 under TOL on a large, a small and a mid-sized gradient and on one whose last
    float4 carries the norm; twice, the same bits."""
    c = dict(case_inputs(n))
    # "tail": the last float4 -- at n4 = 262 145 the one float4 of the second sweep -- carries nearly all of the norm; among random
    # values a float4 that is left out moves the norm by 2e-6 of itself, under any tolerance
    c["tail"] = c["g_small"].clone()
    c["tail"][-4:] = 1.0
    for key in ("g_big", "g_small", "m1", "tail"):
        g = c[key].to(_dev())
        a, b = _norm_once(g), _norm_once(g)
        assert _same_bits(a, b)
        want = grad_norm(c[key])
        err = abs(float(a) - want) / want
        _report(f"grad_norm n {n} {key}: norm {want:.6e} error {err:.3e} bound {TOL:.1e}")
        assert err < TOL, (n, key, err)


@pytest.mark.parametrize("n", [1028, 2097156])
def test_an_all_zero_gradient_changes_nothing(n):
    """norm exactly 0 (coefficient 1 / 1e-6, clamped to 1); parameters and (zero) moments come back bit for bit"""
    c = case_inputs(n)
    zeros = torch.zeros(n)
    p, m, v, norm = _adam_once(c["p"], zeros, zeros, zeros, 1, "clip")
    assert float(norm) == 0.0 and int(_bits(norm)) == 0
    assert _same_bits(p.cpu(), c["p"]) and _same_bits(m.cpu(), zeros) and _same_bits(v.cpu(), zeros)
    p2, m2, v2, _ = _adam_once(c["p"], zeros, zeros, zeros, 1, "clip")
    assert _same_bits(p, p2) and _same_bits(m, m2) and _same_bits(v, v2)


@pytest.mark.parametrize("n", [4, 1028, 2097156])
def test_adam_reads_lr_and_step_from_the_state_block(n):
    """lr and step pushed through ops.StepState, by-value arguments that differ (lr x 10, step + 5): the result is the fp64 step at
    the BLOCK's values, and bit for bit the launch without a block that passes the block's values by value."""
    from transformertts_amd import ops
    c, step = case_inputs(n), 7
    st = ops.StepState(_dev())
    st.push(seed=0x1234567, lr=LR, p_tf=0.25, step=step)
    p, m, v = _adam_twice(c["p"], c["g_big"], c["m1"], c["v1"], step + 5, "clip", lr=LR * 10, st=st.ptr)
    rp, rm, rv, coef = clip_adam_step(c["p"], c["g_big"], c["m1"], c["v1"], step, LR, max_norm=1.0)
    e = {"update": rel(p.double().cpu() - c["p"].double(), rp - c["p"].double()), "exp_avg": rel(m, rm), "exp_avg_sq": rel(v, rv)}
    _report(f"state block n {n} step {step} coef {coef:.3e}: " + " ".join(f"{k} kernel {e[k]:.3e} bound {BOUND[k]:.3e}" for k in MEASURES))
    assert coef < 1.0 and all(e[k] < BOUND[k] for k in MEASURES), e
    q, qm, qv = _adam_twice(c["p"], c["g_big"], c["m1"], c["v1"], step, "clip", lr=LR, st=None)
    assert _same_bits(p, q) and _same_bits(m, qm) and _same_bits(v, qv)
    # the block's other fields are where StepState says they are
    torch.cuda.synchronize()
    words = st.dev.cpu()
    assert int(words[0]) == 0x1234567 and int(words[2]) == step
    assert words.view(torch.float32)[2].item() == torch.tensor(LR, dtype=torch.float32).item() and words.view(torch.float32)[3].item() == 0.25


# ------------------------------------------------------------------------------------------------------ FlatAdam and TrainStep wiring
_SHAPES = [(37, 64), (130,), (5, 3, 7), (1,), (33, 9)]


def _grads(step):
    return [_rand(*s, seed=100 * step + i, scale=(3.0 if step % 2 else 1e-4)) for i, s in enumerate(_SHAPES)]


def _flat_adam(params):
    from transformertts_amd.optim import FlatAdam
    ps = [torch.nn.Parameter(t.detach().clone().to(_dev())) for t in params]
    return ps, FlatAdam(ps, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=1.0)


def _step(ps, opt, step):
    opt.zero_grad()
    for p, g in zip(ps, _grads(step)):
        p.grad.copy_(g.to(_dev()))
    opt.step()


def test_flat_adam_state_dict_restores_step_and_moments_and_loads_twice():
    """Two steps, state_dict() (deep-copied: it hands out the live moment buffers), a fresh FlatAdam over clones of the parameters
    loads the copy, two more steps on both: the same bits in parameters and moments, the same step count.  The same dictionary then
    loads a second time, into a third optimizer, with its step and moments, and still holds its "flat" entry."""
    ps, opt = _flat_adam([_rand(*s, seed=10 + i, scale=0.05) for i, s in enumerate(_SHAPES)])
    for k in (1, 2):
        _step(ps, opt, k)
    sd = copy.deepcopy(opt.state_dict())
    at2 = [t.detach().clone() for t in ps]
    m2, v2 = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    assert float(m2.abs().max()) > 0.0 and float(v2.abs().max()) > 0.0
    ps_b, opt_b = _flat_adam(at2)
    opt_b.load_state_dict(sd)
    assert "flat" in sd and opt_b._step == 2 and _same_bits(opt_b.exp_avg, m2) and _same_bits(opt_b.exp_avg_sq, v2)
    for k in (3, 4):
        _step(ps, opt, k)
        _step(ps_b, opt_b, k)
    assert opt._step == opt_b._step == 4
    assert _same_bits(opt.flat_params, opt_b.flat_params)
    assert _same_bits(opt.exp_avg, opt_b.exp_avg) and _same_bits(opt.exp_avg_sq, opt_b.exp_avg_sq)
    assert not _same_bits(opt.exp_avg, m2)                             # (the two further steps moved them)
    ps_c, opt_c = _flat_adam(at2)
    opt_c.load_state_dict(sd)                                          # the same dictionary object again
    assert "flat" in sd and set(sd["flat"]) == {"step", "exp_avg", "exp_avg_sq"}
    assert opt_c._step == 2 and _same_bits(opt_c.exp_avg, m2) and _same_bits(opt_c.exp_avg_sq, v2)
    for k in (3, 4):
        _step(ps_c, opt_c, k)
    assert opt_c._step == 4 and _same_bits(opt_c.flat_params, opt.flat_params) and _same_bits(opt_c.exp_avg_sq, opt.exp_avg_sq)


# Gradient scale of each of the five steps of test_train_step_update_against_fp64.  The tiny model's own gradient (seed-8 batch,
# fill_state seed 3) has a global norm of 10 to 16 in every step (it moves with the dropout masks), so at scale 1 every step clips;
# d(loss) = 2^-12 on steps 2 and 4 (one eager, one replayed) brings the norm to 3e-3 there.  The fp64 reference decides which steps clipped, from the gradient
# the update consumed.
_GRAD_SCALES = (1.0, 2.0 ** -12, 1.0, 2.0 ** -12, 1.0)


def test_train_step_update_against_fp64():
    """TrainStep(graph=True) on the tiny model, fused_clip_norm 1.0, warm-up 50, dropout on: five steps (two eager, three replayed).
    Each step's update and moments are recomputed in fp64 from the state before it and the gradient it consumed (bucket.flat, zeroed
    only at the start of the next step), with lr = noam_lambda(d_model, 50)(k - 1) and step = k for step k -- the schedule's order
    under LambdaLR (steps 1 and 2 share a rate), the state block's lr and step fields, and the clip, tied to arithmetic outside the
    library."""
    from oracle.ref_model import noam_lambda
    from test_hip_graph import _setup
    from transformertts_amd.step import TrainStep
    from transformertts_amd.workload import synth_batch
    cfg, lm, opt, sch = _setup("tiny", 3, 0)
    assert opt.param_groups[0]["max_grad_norm"] == 1.0 and lm.config["training"]["warmup_steps"] == 50
    batch = {k: v.to("cuda") for k, v in synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=8).items()}
    ts = TrainStep(lm, opt, sch, batch, graph=True, seed=77)
    lam = noam_lambda(cfg["d_model"], 50)
    coefs = []
    for k, scale in enumerate(_GRAD_SCALES, start=1):
        ts._grad_seed.fill_(scale)                                      # d(loss): resident, read by eager and replayed steps alike
        torch.cuda.synchronize()
        p0, m0, v0 = opt.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
        assert opt.param_groups[0]["lr"] == lam(k - 1)
        loss = ts()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and opt._step == k and ts.graphed == (k > 2)
        g = opt.bucket.flat.clone()
        rp, rm, rv, coef = clip_adam_step(p0, g, m0, v0, k, lam(k - 1), BETAS, EPS, 1.0)
        coefs.append(coef)
        e = {"update": rel(opt.flat_params.double().cpu() - p0.double().cpu(), rp - p0.double().cpu()),
             "exp_avg": rel(opt.exp_avg, rm), "exp_avg_sq": rel(opt.exp_avg_sq, rv)}
        _report(f"TrainStep tiny step {k} ({'replayed' if k > 2 else 'eager'}) d(loss) {scale:.3e} norm {grad_norm(g):.4e} coef {coef:.3e} "
                f"lr {lam(k - 1):.4e}: " + " ".join(f"{m} kernel {e[m]:.3e} bound {BOUND[m]:.3e}" for m in MEASURES))
        assert float(rp.sub(p0.double().cpu()).abs().max()) > 0.0
        for m in MEASURES:
            assert e[m] < BOUND[m], (k, m, e[m])
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    assert lam(0) == lam(1) and lam(2) == 2 * lam(1)


# ---------------------------------------------------------------------------------------------------------------------- step head
# The longest utterances come LAST: what a second sweep covers -- the backward's and the mix's from float4 524 288 on (utterance 15
# from frame 714), the forward's from 262 144 on -- then holds valid frames with non-zero expectations, so a loop that stops after
# its first sweep cannot hide behind padding (where an unwritten fresh allocation and the expected zero look alike).
_WRAP = (16, 1700, 80, [1, 2, 33, 64, 129, 300, 511, 512, 777, 900, 1023, 1024, 1025, 1501, 1699, 1700])
_EDGE = (8, 1639, 80, [1, 8, 77, 640, 801, 1200, 1638, 1639])


def _loss_case(B, T, C, lens, which, stop=None):
    """the fused loss and its backward against oracle_loss in fp64; `which`: weights of (total, pred_mel, post_mel, stop) in the
    scalar that is backpropagated, 0 = that output gets no upstream gradient (a NULL pointer in ttts_loss_bwd).  Bounds as in
    tests/test_hip_ops.py::test_loss_kernels: scalars 2e-6 max(1, |ref|), gradients TOL; padded frames exactly zero."""
    from oracle import oracle_loss
    from transformertts_amd.loss import TransformerTTSLoss
    assert len(lens) == B and max(lens) <= T
    pred, post, mel = _rand(B, T, C, seed=1), _rand(B, T, C, seed=2), _rand(B, T, C, seed=4)
    stop = _rand(B, T, seed=3, scale=2.0) if stop is None else stop
    lens_t = torch.tensor(lens, dtype=torch.int64)
    keys = ("total", "pred_mel", "post_mel", "stop")
    pd, qd, sd = [t.double().requires_grad_() for t in (pred, post, stop)]
    ref = oracle_loss({"pred_melspec": pd, "post_melspec": qd, "pred_stop": sd}, mel.double(), lens_t)
    assert all(ref[k].dtype == torch.float64 for k in keys)
    sum(w * ref[k] for w, k in zip(which, keys) if w).backward()
    pg, qg, sg = _g(pred), _g(post), _g(stop)
    out = TransformerTTSLoss(8.0).to(_dev())({"pred_melspec": pg, "post_melspec": qg, "pred_stop": sg}, mel.to(_dev()), lens_t.to(_dev()))
    for k in keys:
        assert abs(out[k].item() - ref[k].item()) < 2e-6 * max(1.0, abs(ref[k].item())), (k, out[k].item(), ref[k].item())
    sum(w * out[k] for w, k in zip(which, keys) if w).backward()
    torch.cuda.synchronize()
    errs = []
    for name, got, want in (("dpred", pg.grad, pd.grad), ("dpost", qg.grad, qd.grad), ("dstop", sg.grad, sd.grad)):
        assert got is not None and torch.isfinite(got).all()
        if want is None:                    # the backpropagated scalar does not depend on this input: exact zeros
            assert float(got.abs().max()) == 0.0, name
            errs.append(0.0)
        else:
            errs.append(rel_l2(got, want))
            assert errs[-1] < TOL, (name, errs[-1])
    for b, n in enumerate(lens):            # padded frames (and the whole of an empty utterance) get exactly zero gradient
        assert float(pg.grad[b, n:].abs().sum()) == 0.0 and float(qg.grad[b, n:].abs().sum()) == 0.0
        assert float(sg.grad[b, n:].abs().sum()) == 0.0
    _report(f"loss ({B},{T},{C}) upstream {which}: " + " ".join(f"{k} {abs(out[k].item() - ref[k].item()):.3e}" for k in keys) +
            " dpred {:.3e} dpost {:.3e} dstop {:.3e}".format(*errs))
    return out, ref


@pytest.mark.parametrize("B,T,C,lens", [_WRAP, _EDGE], ids=["wrap-544000", "edge-262240"])
def test_loss_kernels_where_the_grids_wrap(B, T, C, lens):
    """(16, 1700, 80): 544 000 float4s -- above the 524 288 one sweep of the backward's 2048 blocks covers and twice the 262 144 of
    the forward's 1024; (8, 1639, 80): 262 240, the forward's sweep crossed by 96 float4s, less than one block."""
    n4 = B * T * C // 4
    assert n4 == (544000 if B == 16 else 262240) and (n4 > 2048 * 256 if B == 16 else 0 < n4 - 1024 * 256 < 256)
    _loss_case(B, T, C, lens, (1.0, 0.3, -0.7, 2.0))


def test_loss_kernels_with_an_empty_utterance():
    T = 37
    _loss_case(4, T, 16, [T, 1, 0, 7], (1.0, 0.3, -0.7, 2.0))


@pytest.mark.parametrize("which", [(1.0, 0, 0, 0), (0, 0, 0, 1.0)], ids=["total-only", "stop-only"])
def test_loss_backward_with_missing_upstream_gradients(which):
    """only `total`, only `stop` backpropagated: the other three upstream pointers of ttts_loss_bwd are NULL"""
    _loss_case(4, 300, 80, [300, 211, 95, 1], which)


def test_loss_kernels_on_a_saturated_stop_gate():
    """stop logits drawn at scale 12 with +-30, +-60 and +-90 planted, also at last valid frames (the positive class): the fast
    exponential of softplus_neg and of the backward's sigmoid under the same bounds"""
    B, T, C, lens = 4, 300, 80, [300, 211, 95, 40]
    stop = _rand(B, T, seed=3, scale=12.0)
    planted = [30.0, -30.0, 60.0, -60.0, 90.0, -90.0]
    for i, x in enumerate(planted):
        stop[i % B, 3 + 5 * i] = x                       # inside every utterance (frames 3 .. 28)
    for b, x in zip(range(B), (30.0, -60.0, 90.0, -90.0)):
        stop[b, lens[b] - 1] = x                         # the gate frame
    stop[0, 150], stop[1, 150] = 60.0, -30.0
    out, ref = _loss_case(B, T, C, lens, (1.0, 0.3, -0.7, 2.0), stop=stop)
    assert ref["stop"].item() > 1.0                      # (the saturated terms are the loss)


@pytest.mark.parametrize("p_tf", [0.7, 0.05])
def test_mix_kernel_where_the_grid_wraps(p_tf):
    """(16, 1700, 80) with an injected draw: bit for bit the max-pool restatement of
    test_hip_ops.py::test_block_mask_shim_matches_reference_windowing applied to pred / mel, padded frames exactly zero, and the
    published maxima hold max|out| exactly."""
    from transformertts_amd import ops
    B, T, C, lens = _WRAP
    dev = _dev()
    pred, mel = _rand(B, T, C, seed=1), _rand(B, T, C, seed=4)
    u = torch.rand(B, 1, T, generator=torch.Generator().manual_seed(5))
    lens_t = torch.tensor(lens, dtype=torch.int64)
    mask = F.max_pool1d((u < (1 - p_tf)).float(), kernel_size=8, stride=1, padding=4).squeeze(1).bool().unsqueeze(-1)[:, :T, :]
    valid = (torch.arange(T)[None, :] < lens_t[:, None]).unsqueeze(-1)
    want = torch.where(valid, torch.where(mask, pred, mel), torch.zeros(()))
    frac = float(mask.float().mean())
    # a frame keeps the truth only if all 8 draws of its window are >= 1 - p_tf: 0.7^8 = 5.8 % of the frames, 0.05^8 = none
    assert (0.90 < frac < 0.98) if p_tf == 0.7 else frac == 1.0
    outs = [ops.sched_sampling_mix(pred.to(dev), mel.to(dev), u.view(B, T).to(dev), lens_t.to(dev), p_tf, 8) for _ in range(2)]
    out = outs[0]
    assert _same_bits(out.cpu(), want) and _same_bits(outs[1], out)
    for b, n in enumerate(lens):
        assert float(out[b, n:].abs().sum()) == 0.0
    am = out._ttts_amax
    assert am.numel() == ops.AMAX_SLOTS and _same_bits(am.max().view(1), out.abs().max().view(1))
    assert _same_bits(am.max().view(1).cpu(), want.abs().max().view(1))
