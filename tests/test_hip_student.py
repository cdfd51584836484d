"""Training the student on the device (csrc/student_loss.hip through transformertts_amd/student.py): `mel_loss` against the fp64
oracle of tests/student_reference.py under the project's kernel bound (TOL of tests/test_hip_modes.py, conftest.rel_l2), at the
smallest shapes that reach every path -- one frame, a zero length, a target longer and shorter than the prediction, frame counts
around the chunk of one workgroup, one workgroup more than the finishing launch takes in a sweep, one chunk more than the grid's
cap, strided views.  NaN sits at and behind every n_b of pred and of target and between the rows of the views throughout.  Then
`FastSpeech2Loss`, `StudentTrainStep` on the student fixture of tests/test_hip_fft.py (rebuilt here) against fp64 -- the gradient
under the rule of tests/test_hip_model.py, three clipped Adam steps under tests/optim_reference.py's BOUND -- and
`distillation_targets` against its three calls made by hand.
Measured values: parity_reports/student_margin.txt (as measured on one MI355X: tests/reports/student_margin.txt)."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_l2
from fft_reference import student_ref
from optim_reference import BETAS, BOUND, EPS, clip_adam_step, grad_norm, rel
from student_reference import mel_case, mel_loss_grad_ref, mel_loss_ref, mel_loss_stock
from test_hip_dropout_parity import REPORT_DIR
from test_hip_modes import TOL
from transformertts_amd import _lib as _library
from transformertts_amd.student import FastSpeech2Loss, StudentTrainStep, distillation_targets, mel_loss  # noqa: F401 -- no feature, no tests

_lib = _library.load()                                                # raises when the library lacks the entries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, SWEEP, CAP = _lib.ttts_mel_loss_rows(), _lib.ttts_mel_loss_sweep(), _lib.ttts_mel_loss_max_workgroups()
assert TOL == 5e-6
W, EXTRA, G = (0.8, 0.6), 0.37, (0.3, -0.7, 0.5, 1.1)                 # weights, the extra scalar, the four upstream gradients
KEYS = ("mae", "mse", "mel", "total")

# name -> B, T, Tt, M, pred_lens, target_lens, (row, batch) strides of pred and of target or None
CASES = {
    "one": (1, 1, 1, 4, (1,), (1,), None),
    "zero_length": (3, 70, 70, 16, (70, 12, 0), (70, 12, 0), None),
    "target_longer_and_shorter": (2, 33, 40, 80, (33, 20), (40, 17), None),
    "the_mirror": (2, 40, 33, 80, (40, 17), (33, 20), None),
    "chunk_minus_one": (2, ROWS - 1, ROWS - 1, 8, (ROWS - 1, 5), (ROWS - 1, 9), None),
    "chunk": (2, ROWS, ROWS, 8, (ROWS, 5), (ROWS, 9), None),
    "chunk_plus_one": (2, ROWS + 1, ROWS + 1, 8, (ROWS + 1, 5), (ROWS + 1, 9), None),
    "sweep_plus_one": (1, ROWS * SWEEP + 1, ROWS * SWEEP + 1, 4, (ROWS * SWEEP + 1,), (ROWS * SWEEP + 1,), None),   # SWEEP + 1 workgroups
    "cap_plus_one": (1, ROWS * CAP + 1, ROWS * CAP + 1, 4, (ROWS * CAP + 1,), (ROWS * CAP + 1,), None),            # workgroup 0 takes two chunks
    "strided": (2, 33, 40, 80, (33, 20), (40, 17), ((84, 33 * 84 + 8), (88, 40 * 88 + 4))),
}


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/student_margin.txt", "a") as f:
        f.write(line + "\n")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _view(a, strides):
    """a (B, rows, M) numpy array on the device: contiguous, or a view of a wider buffer whose gaps hold NaN"""
    t = _dev(a)
    if strides is None:
        return t
    ld_row, ld_batch = strides
    store = torch.full((a.shape[0] * ld_batch,), float("nan"), device=DEV)
    view = store.as_strided(a.shape, (ld_batch, ld_row, 1))
    view.copy_(t)
    return view


@functools.lru_cache(maxsize=None)
def _case(name, zeros=False):
    """the fixture and the oracle's losses and gradient (computed once, never modified)"""
    B, T, Tt, M, pl, tl, _ = CASES[name]
    c = dict(mel_case(B, T, Tt, M, pl, tl, zeros=zeros))
    c["ref"] = mel_loss_ref(c["pred"], pl, c["target"], tl, W, EXTRA)
    c["grad"] = mel_loss_grad_ref(c["pred"], pl, c["target"], tl, W, G)
    return c


def _run(name, g=G, scale=1.0, weights=W, extra=EXTRA, zeros=False):
    """mel_loss on the case and its gradient under the upstream gradients g * scale -> (dict of the outputs, dpred, d extra)"""
    c = _case(name, zeros)
    strides = CASES[name][6] or (None, None)
    pred = _view(c["pred"], strides[0]).requires_grad_(True)
    target = _view(c["target"], strides[1])
    ex = None if extra is None else torch.tensor(extra, device=DEV, requires_grad=True)
    out = mel_loss(pred, _dev(c["pred_lens"]), target, _dev(c["target_lens"]), weights, ex)
    used = [(out[k], torch.tensor(v * scale, dtype=torch.float32, device=DEV)) for k, v in zip(KEYS, g) if v is not None]
    grads = torch.autograd.grad([o for o, _ in used], [pred] + ([] if ex is None else [ex]), [v for _, v in used], allow_unused=True)
    torch.cuda.synchronize()
    return out, grads[0], (grads[1] if ex is not None else None)


def _zeros_behind(dpred, n):
    return all(not bool(_bits(dpred[b, k:]).any()) for b, k in enumerate(n))     # bit for bit: +0.0, not -0.0


# ------------------------------------------------------------------------------------------------ mel_loss against fp64
@pytest.mark.parametrize("scale", [1.0, 2e-7])
@pytest.mark.parametrize("name", list(CASES))
def test_mel_loss_against_fp64(name, scale):
    c = _case(name)
    out, dpred, dextra = _run(name, scale=scale)
    errs = {k: rel_l2(out[k], c["ref"][k]) for k in KEYS}
    errs["dpred"] = rel_l2(dpred, c["grad"] * scale)
    _report(f"mel_loss {name} (upstream x {scale:g}): " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert int(out["frames"]) == c["ref"]["frames"] == sum(c["n"]) and out["frames"].dtype == torch.int64
    assert not any(bool(torch.isnan(out[k])) for k in KEYS) and not bool(torch.isnan(dpred).any())
    assert dpred.shape == c["pred"].shape and dpred.is_contiguous() and _zeros_behind(dpred, c["n"])
    assert all(v < TOL for v in errs.values()), errs
    assert _same_bits(dextra, torch.tensor(G[3] * scale, dtype=torch.float32))         # the gradient reaching extra is g_total
    total, mel = float(out["total"].detach()), float(out["mel"].detach())
    assert abs(total - mel - float(np.float32(EXTRA))) <= 2.0 ** -24 * abs(total)    # total - mel is extra to one fp32 rounding
    if scale != 1.0:
        return
    again, dagain, _ = _run(name)                                     # the same bits on every call
    assert all(_same_bits(again[k], out[k]) for k in KEYS) and _same_bits(dagain, dpred)
    bare, _, _ = _run(name, extra=None)                               # extra NULL: total is mel itself
    assert _same_bits(bare["total"], bare["mel"]) and _same_bits(bare["mel"], out["mel"])


def test_no_frames_at_all_gives_exact_zeros():
    B, T, Tt, M = 3, 20, 24, 8
    nan = float("nan")
    pred = torch.full((B, T, M), nan, device=DEV, requires_grad=True)
    target = torch.full((B, Tt, M), nan, device=DEV)
    for pl, tl in (((0, 0, 0), (0, 0, 0)), ((20, 0, -5), (0, 24, 7))):
        out = mel_loss(pred, torch.tensor(pl, device=DEV), target, torch.tensor(tl, device=DEV), W)
        dpred, = torch.autograd.grad([out[k] for k in KEYS], [pred], [torch.ones((), device=DEV)] * 4)
        assert all(_same_bits(out[k], np.float32(0)) for k in KEYS) and int(out["frames"]) == 0
        assert not bool(_bits(dpred).any())


def test_sign_of_zero_is_zero():
    name = "target_longer_and_shorter"
    c = _case(name, True)
    out, dpred, _ = _run(name, g=(None, None, None, 1.0), weights=(1.0, 0.0), extra=None, zeros=True)
    planted = torch.from_numpy(c["planted"])
    assert int(planted.sum()) > 0.2 * sum(c["n"]) * 80
    d = torch.from_numpy(np.nan_to_num(c["pred"][:, :33]) - np.nan_to_num(c["target"][:, :33]))
    got = dpred.cpu()
    assert not bool(_bits(got[planted]).any())                        # exactly 0 where pred == target
    rest = torch.zeros_like(planted)
    for b, k in enumerate(c["n"]):
        rest[b, :k] = True
    rest &= ~planted
    mags = got[rest].abs().unique()
    assert len(mags) == 1 and float(mags[0]) == float(np.float32(1.0) / np.float32(sum(c["n"]) * 80))    # one magnitude
    assert torch.equal(torch.sign(got[rest]), torch.sign(d[rest]))                                        # with the sign of pred - target
    assert _zeros_behind(dpred, c["n"])
    assert rel_l2(out["mae"], mel_loss_ref(c["pred"], c["pred_lens"], c["target"], c["target_lens"])["mae"]) < TOL


@pytest.mark.parametrize("which", range(4))
def test_each_upstream_gradient_alone_and_null(which):
    name = "target_longer_and_shorter"
    c = _case(name)
    alone = tuple(1.7 if k == which else None for k in range(4))      # the other three are NULL at the entry
    _, dpred, dextra = _run(name, g=alone)
    as_zeros = tuple(1.7 if k == which else 0.0 for k in range(4))    # ... which counts as 0: the same bits as explicit zeros
    _, dzeros, _ = _run(name, g=as_zeros)
    want = mel_loss_grad_ref(c["pred"], c["pred_lens"], c["target"], c["target_lens"], W, as_zeros)
    assert rel_l2(dpred, want) < TOL and _same_bits(dpred, dzeros) and _zeros_behind(dpred, c["n"])
    assert (dextra is None) == (which != 3) and (which != 3 or _same_bits(dextra, np.float32(1.7)))
    without = tuple(None if k == which else v for k, v in enumerate(G))
    _, dpred, _ = _run(name, g=without)
    want = mel_loss_grad_ref(c["pred"], c["pred_lens"], c["target"], c["target_lens"], W, tuple(0.0 if v is None else v for v in without))
    assert rel_l2(dpred, want) < TOL


def test_a_captured_call_replayed_on_other_inputs_and_lengths():
    B, T, Tt, M = 2, 33, 40, 80
    a, b = mel_case(B, T, Tt, M, (33, 20), (40, 17)), mel_case(B, T, Tt, M, (9, 33), (30, 40), seed=3)
    pred, target = _dev(a["pred"]), _dev(a["target"])
    pl, tl = _dev(a["pred_lens"]), _dev(a["target_lens"])
    extra, gt = torch.tensor(EXTRA, device=DEV), torch.tensor(0.5, device=DEV)

    def call(p, t, l1, l2):
        p = p.detach().requires_grad_(True)
        out = mel_loss(p, l1, t, l2, W, extra)
        return out, torch.autograd.grad(out["total"], p, gt)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # (warm-up: the library is loaded, the allocator primed)
        call(pred, target, pl, tl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got, dgot = call(pred, target, pl, tl)
    seen = []
    for c in (a, b):
        for dst, src in ((pred, c["pred"]), (target, c["target"]), (pl, c["pred_lens"]), (tl, c["target_lens"])):
            dst.copy_(_dev(src))
        graph.replay()
        torch.cuda.synchronize()
        eager, deager = call(_dev(c["pred"]), _dev(c["target"]), _dev(c["pred_lens"]), _dev(c["target_lens"]))
        assert all(_same_bits(got[k], eager[k]) for k in KEYS) and _same_bits(dgot, deager) and int(got["frames"]) == sum(c["n"])
        assert rel_l2(got["total"], mel_loss_ref(c["pred"], c["pred_lens"], c["target"], c["target_lens"], W, EXTRA)["total"]) < TOL
        seen.append(float(got["total"].detach()))
    assert seen[0] != seen[1]                                         # the replay did follow the inputs


# ------------------------------------------------------------------------------------------------ the student fixture
STUDENT = dict(n_vocab=20, d_model=64, encoder_layers=2, decoder_layers=2, n_head=2, d_hidden=96, n_mels=16)
STUDENT_LENS, STUDENT_PMAX = (12, 7, 3), 12
MEL_W, VAR_W = (1.0, 0.5), (1.0, 0.5, 2.0)


def _student(dropout=0.0):
    from transformertts_amd import FastSpeech2Student, KernelVariancePredictor
    torch.manual_seed(23)
    m = FastSpeech2Student(**STUDENT, dropout=dropout, predictor=lambda d: KernelVariancePredictor(d, hidden=96, dropout=dropout), n_bins=8,
                           min_duration=1)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m


@functools.lru_cache(maxsize=None)
def _batch(seed=8):
    """3 utterances of 12, 7, 3 phonemes, durations 1 .. 4, the mel as long as the longest sum; NaN behind every length"""
    B, P = len(STUDENT_LENS), STUDENT_PMAX
    rng = np.random.default_rng(seed)
    phoneme = torch.from_numpy(rng.integers(1, STUDENT["n_vocab"], (B, P)))
    dur = torch.from_numpy(rng.integers(1, 5, (B, P)))
    pitch = torch.from_numpy(rng.uniform(70, 500, (B, P)).astype(np.float32))
    energy = torch.from_numpy(rng.uniform(0, 1, (B, P)).astype(np.float32))
    pl = torch.tensor(STUDENT_LENS)
    valid = torch.arange(P)[None, :] < pl[:, None]
    ml = torch.where(valid, dur, torch.zeros_like(dur)).sum(1)
    mel = torch.from_numpy(rng.standard_normal((B, int(ml.max()), STUDENT["n_mels"])).astype(np.float32))
    for b in range(B):
        dur[b, STUDENT_LENS[b]:], pitch[b, STUDENT_LENS[b]:], energy[b, STUDENT_LENS[b]:] = 0x7FF8000000000000, float("nan"), float("nan")
        mel[b, int(ml[b]):] = float("nan")
    return dict(phoneme=phoneme, phoneme_lens=pl, melspec=mel, melspec_lens=ml, durations=dur, pitch=pitch, energy=energy)


def _on_device(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _stepper(sd, dropout=0.0, seed=0, accumulate=1, schedule=False, max_grad_norm=0.0):
    from oracle.ref_model import noam_lambda
    from transformertts_amd.optim import FlatAdam
    m = _student(dropout)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    opt = FlatAdam(m.parameters(), lr=1.0 if schedule else 1e-3, max_grad_norm=max_grad_norm)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, noam_lambda(STUDENT["d_model"], 50)) if schedule else None
    return StudentTrainStep(m, opt, sched, FastSpeech2Loss(MEL_W, VAR_W), seed=seed, accumulate=accumulate), m, opt


def _restated_loss(out, batch, dev):
    """VarianceLoss's three masked means and the mel loss in out's dtype, from stock torch operations (fp64: through the oracle)"""
    dt = out["melspec"].dtype
    P = batch["durations"].shape[1]
    v = torch.arange(P, device=dev)[None, :] < batch["phoneme_lens"].to(dev)[:, None]
    n = v.sum().to(dt)
    zero = out["melspec"].new_zeros(())
    dur = torch.where(v, batch["durations"].to(dev), torch.zeros_like(batch["durations"].to(dev)))
    targets = (("log_duration", torch.log(dur.to(dt) + 1)), ("pitch", torch.nan_to_num(batch["pitch"].to(dev)).to(dt)),
               ("energy", torch.nan_to_num(batch["energy"].to(dev)).to(dt)))
    terms = [(torch.where(v, out[k] - t, zero) ** 2).sum() / n for k, t in targets]
    var = (VAR_W[0] * terms[0] + VAR_W[1] * terms[1]) + VAR_W[2] * terms[2]
    if dt == torch.float64:
        mel = mel_loss_ref(out["melspec"], out["mel_lens"].tolist(), batch["melspec"], batch["melspec_lens"].tolist(), MEL_W, var)
    else:
        mel = mel_loss_stock(out["melspec"], out["mel_lens"], torch.nan_to_num(batch["melspec"].to(dev)), batch["melspec_lens"].to(dev), MEL_W, var)
    return {"total": mel["total"], "mel": mel["mel"], "mae": mel["mae"], "mse": mel["mse"], "duration": terms[0], "pitch": terms[1],
            "energy": terms[2]}


def _held_to_stock(tag, kernel, stock, ref):
    """the rule of tests/test_hip_model.py: below twice the stock fp32 path's error against the same fp64, and below 1e-4"""
    bad = {}
    for k in ref:
        e, e32 = rel_l2(kernel[k], ref[k]), rel_l2(stock[k], ref[k])
        _report(f"{tag} {k}: kernels {e:.3e} stock fp32 {e32:.3e}")
        if not (e < 2.0 * e32 and e < 1e-4):
            bad[k] = (e, e32)
    assert not bad, bad


def _flat_by_name(m, opt):
    """name -> the parameter's slice of the gradient bucket"""
    names = {id(p): k for k, p in m.named_parameters()}
    return {names[id(p)]: opt.bucket.flat[off:off + p.numel()].view_as(p) for p, off in zip(opt.bucket.params, opt.bucket.offsets)}


def test_the_loss_module_is_the_two_losses_called_by_hand():
    from transformertts_amd import VarianceLoss
    m = _student().to(DEV).train()
    b = _on_device(_batch())
    out = m(b["phoneme"], b["phoneme_lens"], b["durations"], b["pitch"], b["energy"], max_len=b["melspec"].size(1))
    got = FastSpeech2Loss(MEL_W, VAR_W)(out, b["melspec"], b["melspec_lens"], b["durations"], b["pitch"], b["energy"], b["phoneme_lens"])
    var = VarianceLoss(VAR_W)(out, b["durations"], b["pitch"], b["energy"], b["phoneme_lens"])
    mel = mel_loss(out["melspec"], out["mel_lens"], b["melspec"], b["melspec_lens"], MEL_W, extra=var["total"])
    assert tuple(sorted(got)) == ("duration", "energy", "frames", "mae", "mel", "mse", "pitch", "total")
    for k in ("total", "mel", "mae", "mse", "frames"):
        assert _same_bits(got[k], mel[k]), k
    for k in ("duration", "pitch", "energy"):
        assert _same_bits(got[k], var[k]), k
    assert int(got["frames"]) == int(b["melspec_lens"].sum()) and bool(torch.isfinite(got["total"]))
    # extra is part of total: total - mel is the variance total to one fp32 rounding, and its gradient reaches the predictors
    total, part, extra = (float(t.detach()) for t in (got["total"], got["mel"], var["total"]))
    assert abs(total - part - extra) <= 2.0 ** -24 * abs(total)
    got["total"].backward()
    assert bool(m.adaptor.duration_predictor.out.weight.grad.any()) and bool(m.mel_linear.weight.grad.any())


def test_the_first_steps_gradient_against_fp64_and_the_stock_fp32_path():
    sd = {k: v.detach().clone() for k, v in _student().state_dict().items()}
    batch = _batch()
    step, m, opt = _stepper(sd)
    names = [k for k, _ in m.named_parameters()]
    T = batch["melspec"].size(1)
    res = {}
    for tag, dtype, dev in (("ref", torch.float64, "cpu"), ("stock", torch.float32, DEV)):
        p = {k: (v.to(dev, dtype) if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
        for k in names:
            p[k].requires_grad_(True)
        dur = torch.where(torch.arange(STUDENT_PMAX)[None, :] < batch["phoneme_lens"][:, None], batch["durations"], torch.zeros(()).long())
        out = student_ref(p, STUDENT, batch["phoneme"].to(dev), STUDENT_LENS, dur.to(dev), torch.nan_to_num(batch["pitch"]).to(dev),
                          torch.nan_to_num(batch["energy"]).to(dev), T)
        losses = _restated_loss(out, batch, dev)
        gr = torch.autograd.grad(losses["total"], [p[k] for k in names])
        res[tag] = dict({k: v.detach() for k, v in losses.items()}, **dict(zip(names, gr)))
    got = step(_on_device(batch))
    torch.cuda.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and not v.requires_grad for v in got.values())
    assert opt._step == 1 and step.index == 1 and step.micro == 0 and int(got["frames"]) == int(batch["melspec_lens"].sum())
    kernel = dict({k: got[k] for k in res["ref"] if k not in names}, **_flat_by_name(m, opt))
    assert not any(bool(torch.isnan(v).any()) for v in kernel.values())
    _held_to_stock("StudentTrainStep first step", kernel, res["stock"], res["ref"])


def test_three_steps_under_the_noam_schedule_against_fp64():
    from oracle.ref_model import noam_lambda
    sd = {k: v.detach().clone() for k, v in _student().state_dict().items()}
    step, m, opt = _stepper(sd, schedule=True, max_grad_norm=1.0, seed=77)
    lam = noam_lambda(STUDENT["d_model"], 50)
    batch = _on_device(_batch())
    for k in (1, 2, 3):
        torch.cuda.synchronize()
        p0, m0, v0 = opt.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
        assert opt.param_groups[0]["lr"] == lam(k - 1)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = step(batch)
        assert not [w for w in seen if "lr_scheduler.step()" in str(w.message)]   # the optimizer steps first, then the schedule
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got["total"])) and opt._step == k and step.index == k
        assert step.state.dev.view(torch.float32)[2].item() == np.float32(lam(k - 1)) and int(step.state.dev[2]) == k   # the state block
        g = opt.bucket.flat.clone()                                   # zeroed only at the start of the next step
        rp, rm, rv, coef = clip_adam_step(p0, g, m0, v0, k, lam(k - 1), BETAS, EPS, 1.0)
        e = {"update": rel(opt.flat_params.double().cpu() - p0.double().cpu(), rp - p0.double().cpu()),
             "exp_avg": rel(opt.exp_avg, rm), "exp_avg_sq": rel(opt.exp_avg_sq, rv)}
        _report(f"StudentTrainStep step {k} norm {grad_norm(g):.4e} coef {coef:.3e} lr {lam(k - 1):.4e}: " +
                " ".join(f"{q} kernel {e[q]:.3e} bound {BOUND[q]:.3e}" for q in e))
        assert float((opt.flat_params - p0).abs().max()) > 0.0        # the parameters moved
        for q in e:
            assert e[q] < BOUND[q], (k, q, e[q])
    assert lam(0) == lam(1) and lam(2) == 2 * lam(1)                  # steps 1 and 2 share a rate, step 3 does not


def test_dropout_is_reproducible_from_the_seed_and_fresh_every_step():
    from transformertts_amd.step import _step_seed
    sd = {k: v.detach().clone() for k, v in _student(0.2).state_dict().items()}
    batch = _on_device(_batch())
    flats, firsts = [], []
    for seed in (5, 5, 6):
        step, m, opt = _stepper(sd, dropout=0.2, seed=seed)
        losses = []
        for k in range(3):
            losses.append(step(batch)["total"].clone())
            word = _step_seed(seed, k)
            assert int(step.state.dev[0]) == (word - (1 << 64) if word >= (1 << 63) else word)   # the seed word of step k was pushed
        torch.cuda.synchronize()
        flats.append(opt.flat_params.clone())
        firsts.append(losses[0])
    assert _same_bits(flats[0], flats[1]) and _same_bits(firsts[0], firsts[1])
    assert not _same_bits(flats[0], flats[2]) and not _same_bits(firsts[0], firsts[2])
    assert len({_step_seed(5, k) for k in range(3)}) == 3


def test_accumulating_two_equal_halves_gives_one_halfs_gradient():
    sd = {k: v.detach().clone() for k, v in _student().state_dict().items()}
    batch = _on_device(_batch())
    one, _, opt1 = _stepper(sd)
    one(batch)
    two, _, opt2 = _stepper(sd, accumulate=2)
    two(batch)
    assert opt2._step == 0 and two.micro == 1 and two.index == 1      # the optimizer waits for the window's last micro-batch
    half = opt2.bucket.flat.clone()
    two(batch)
    torch.cuda.synchronize()
    assert opt2._step == 1 and two.micro == 0 and two.index == 2 and opt1._step == 1
    e = rel_l2(opt2.bucket.flat, opt1.bucket.flat)
    _report(f"StudentTrainStep accumulate=2 over two equal halves against accumulate=1: gradient {e:.3e}")
    assert e < TOL                                                    # not bits: the sum of the halves rounds
    assert rel_l2(half * 2, opt1.bucket.flat) < TOL and rel_l2(opt2.flat_params, opt1.flat_params) < TOL


def test_a_step_reads_nothing_back_to_the_host():
    sd = {k: v.detach().clone() for k, v in _student(0.2).state_dict().items()}
    step, m, opt = _stepper(sd, dropout=0.2, schedule=True, max_grad_norm=1.0)
    batch = _on_device(_batch())
    step(batch)                                                       # builds the lazy caches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step(batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got["total"])) and opt._step == 2


# ------------------------------------------------------------------------------------------------ targets from a teacher
def test_distillation_targets_are_the_three_calls_composed_by_hand():
    from oracle import synth_batch
    from pitch_reference import SMALL, glide_signal
    from test_hip_model import _build
    from test_hip_pitch import _config
    from transformertts_amd import PitchEnergy, phoneme_average, teacher_durations
    cfg, teacher = _build("tiny", 11)
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    args = [batch[k].to(DEV) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    hop = SMALL["hop_length"]
    n = [(int(t) - 1) * hop + hop // 2 for t in batch["melspec_lens"]]            # 1 + n // hop frames: the mel's
    n[1] += 2 * hop                                                               # ... and two frames more: melspec_lens is the smaller
    wave = np.zeros((3, max(n)), np.float32)
    for b, k in enumerate(n):
        wave[b, :k] = glide_signal(k, SMALL, 60 + b)
    wave, wave_lens = torch.from_numpy(wave).to(DEV), torch.tensor(n, device=DEV)
    pe = PitchEnergy(_config(SMALL), fmin=SMALL["fmin"], fmax=SMALL["fmax"], frame_length=SMALL["frame_length"], window=SMALL["window"], device=DEV)
    got = distillation_targets(teacher, *args, wave, wave_lens, pe, method="mas")
    d = teacher_durations(teacher, *args, method="mas")
    fr = pe(wave, wave_lens)
    frames = torch.minimum(fr["frames"], args[3])
    assert int(fr["frames"][1]) == int(args[3][1]) + 2 and torch.equal(frames, args[3])
    want = {"durations": d["durations"], "valid": d["valid"], "focus_rate": d["focus_rate"],
            "pitch": phoneme_average(fr["f0"], d["durations"], args[2], frames, mask=fr["voiced"])["mean"],
            "energy": phoneme_average(fr["energy"], d["durations"], args[2], frames)["mean"]}
    assert tuple(sorted(got)) == tuple(sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and _same_bits(got[k], want[k]), k
    valid = got["valid"].cpu()
    total = torch.where(torch.arange(12, device=DEV)[None, :] < args[2][:, None], got["durations"], torch.zeros_like(got["durations"])).sum(1)
    assert bool(valid.any()) and torch.equal(total.cpu()[valid], batch["melspec_lens"][valid])
    assert bool(got["pitch"].gt(0).any()) and bool(got["energy"].gt(0).any())
