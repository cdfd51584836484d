"""Training the student (csrc/student_loss.hip, transformertts_amd/student.py): the fp64 oracle of tests/student_reference.py
against torch's own l1_loss / mse_loss on the selected elements and its closed-form gradient against autograd; every refusal of
the three entry points and of the Python checks with its message, before any launch; the header, the bindings and the exports;
the synthetic student batch; what StudentTrainStep refuses.  Host logic only, no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

from student_reference import MIN_DIFF, counted_diffs, frames_ref, mel_case, mel_loss_grad_ref, mel_loss_ref, mel_loss_stock

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_mel_loss_rows", "ttts_mel_loss_sweep", "ttts_mel_loss_max_workgroups", "ttts_mel_loss_workspace_bytes", "ttts_mel_loss_fwd",
       "ttts_mel_loss_bwd")
EXPORTS = ("mel_loss", "FastSpeech2Loss", "StudentTrainStep", "distillation_targets")


def test_the_header_declares_each_entry_point_once_and_the_exports_agree():
    from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p
    from transformertts_amd import _lib, fft, predictor, student, variance, workload
    import transformertts_amd
    P, I, L, F, Z = c_void_p, c_int, c_int64, c_float, c_size_t
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    for name in NEW:
        decls = re.findall(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M)
        assert len(decls) == 1, f"{name} must be declared exactly once in ttts_hip.h, found {len(decls)}"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        n_args = 0 if decls[0].strip() == "void" else len(decls[0].split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["ttts_mel_loss_workspace_bytes"] == (Z, [I, I, I, I])
    assert _lib.SIGNATURES["ttts_mel_loss_fwd"] == (I, [P, L, L, P, L, L, P, P, I, I, I, I, F, F, P, P, P, P, Z, P])
    assert _lib.SIGNATURES["ttts_mel_loss_bwd"] == (I, [P, L, L, P, L, L, P, P, I, I, I, I, F, F, P, P, P, P, P, P])
    assert lib.ttts_abi_version() == 24                               # additive
    for name in EXPORTS:
        assert getattr(transformertts_amd, name) is getattr(student, name) and name in transformertts_amd.__all__
    assert transformertts_amd.synth_student_batch is workload.synth_student_batch and "synth_student_batch" in transformertts_amd.__all__
    assert tuple(student.__all__) == EXPORTS
    assert "mel_loss" not in fft.__all__ + variance.__all__ + predictor.__all__
    rows, sweep, cap = lib.ttts_mel_loss_rows(), lib.ttts_mel_loss_sweep(), lib.ttts_mel_loss_max_workgroups()
    assert (rows, sweep, cap) == (32, 256, 2048)
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "student_loss.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.replace("__ATOMIC_", "") and "hipMalloc" not in code and "hipMemcpy" not in code
    assert student.MAX_FRAMES == 1 << 20 and "ML_MAX_T = 1 << 20" in src and f"ML_MAX_M = {student.MAX_MELS}" in src
    # the workspace: two floats per workgroup, the workgroups a function of the shapes alone, capped
    ws = lib.ttts_mel_loss_workspace_bytes
    assert ws(1, 1, 1, 4) == 8 and ws(64, 870, 870, 80) == 64 * 28 * 8 and ws(64, 870, 33, 80) == 64 * 2 * 8
    assert ws(1, rows * sweep + 1, rows * sweep + 1, 4) == (sweep + 1) * 8
    assert ws(1, rows * cap + 1, rows * cap + 1, 4) == cap * 8 == ws(65535, 1 << 20, 1 << 20, 4096)
    assert ws(0, 1, 1, 4) == ws(1, 0, 1, 4) == ws(1, 1, 0, 4) == ws(1, 1, 1, 6) == ws(1, 1, 1, 4100) == ws(1, (1 << 20) + 1, 1, 4) == 0


# ------------------------------------------------------------------------------------------------ the oracle
CASES = {"ragged": (3, 11, 9, 8, (11, 4, 0), (9, 6, 5)), "mirror": (2, 9, 11, 8, (9, 5), (11, 2)), "one": (1, 1, 1, 4, (1,), (1,)),
         "past_the_rows": (2, 5, 5, 4, (9, -3), (5, 5))}


def _selected(case):
    """the counted elements of both operands, as torch.masked_select gives them in fp64"""
    pred, target = torch.from_numpy(case["pred"]).double(), torch.from_numpy(case["target"]).double()
    rows = min(pred.shape[1], target.shape[1])
    keep = (torch.arange(rows)[None, :] < torch.tensor(case["n"])[:, None])[:, :, None].expand(-1, -1, pred.shape[2])
    return torch.masked_select(pred[:, :rows], keep), torch.masked_select(target[:, :rows], keep)


@pytest.mark.parametrize("name", list(CASES))
def test_the_oracle_is_torchs_l1_and_mse_on_the_selected_elements(name):
    B, T, Tt, M, pl, tl = CASES[name]
    c = mel_case(B, T, Tt, M, pl, tl)
    assert c["n"] == frames_ref(pl, tl, T, Tt) and all(0 <= k <= min(T, Tt) for k in c["n"])
    assert np.isnan(c["pred"]).sum() == sum(T - k for k in c["n"]) * M and np.isnan(c["target"]).sum() == sum(Tt - k for k in c["n"]) * M
    assert float(np.abs(counted_diffs(c)).min()) >= MIN_DIFF            # away from the kink of |d|
    p, t = _selected(c)
    w, extra = (0.8, 0.6), 0.37
    ref = mel_loss_ref(c["pred"], pl, c["target"], tl, w, extra)
    l1, l2 = torch.nn.functional.l1_loss(p, t), torch.nn.functional.mse_loss(p, t)
    assert ref["frames"] == sum(c["n"]) == p.numel() // M
    assert abs(float(ref["mae"] - l1)) <= 1e-12 * float(l1) and abs(float(ref["mse"] - l2)) <= 1e-12 * float(l2)
    assert abs(float(ref["mel"]) - (0.8 * float(l1) + 0.6 * float(l2))) <= 1e-12 and abs(float(ref["total"] - ref["mel"]) - extra) <= 1e-12
    assert not any(bool(torch.isnan(ref[k])) for k in ("mae", "mse", "mel", "total"))
    # the stock restatement agrees in fp64 (it is the yardstick of the device tests and of the bench)
    stock = mel_loss_stock(torch.from_numpy(c["pred"]).double(), pl, torch.from_numpy(c["target"]).double(), tl, w, extra)
    assert all(abs(float(stock[k] - ref[k])) <= 1e-12 * abs(float(ref[k])) for k in ("mae", "mse", "mel", "total"))
    assert int(stock["frames"]) == ref["frames"]


@pytest.mark.parametrize("name", list(CASES))
def test_the_closed_form_gradient_is_autograds(name):
    B, T, Tt, M, pl, tl = CASES[name]
    c = mel_case(B, T, Tt, M, pl, tl)
    w = (0.8, 0.6)
    for g in ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.3, -0.7, 0.5, 1.1)):
        pred = torch.from_numpy(np.nan_to_num(c["pred"])).double().requires_grad_(True)
        extra = torch.tensor(0.37, dtype=torch.float64, requires_grad=True)
        out = mel_loss_ref(pred, pl, np.nan_to_num(c["target"]), tl, w, extra)
        (g[0] * out["mae"] + g[1] * out["mse"] + g[2] * out["mel"] + g[3] * out["total"]).backward()
        want = mel_loss_grad_ref(c["pred"], pl, c["target"], tl, w, g)
        assert not bool(torch.isnan(want).any())
        scale = float(pred.grad.abs().max())
        assert float((want - pred.grad).abs().max()) <= 1e-11 * scale, (name, g)
        assert float(extra.grad) == g[3]
        for b, k in enumerate(c["n"]):
            assert bool((want[b, k:] == 0).all())


def test_sign_of_zero_is_zero_in_the_oracle_as_in_torch():
    c = mel_case(2, 9, 9, 8, (9, 5), (9, 7), zeros=True)
    assert c["planted"].sum() > 0.15 * sum(c["n"]) * 8
    d = np.nan_to_num(c["pred"]) - np.nan_to_num(c["target"])
    assert bool((d[c["planted"]] == 0).all())
    pred = torch.from_numpy(np.nan_to_num(c["pred"])).double().requires_grad_(True)
    mel_loss_ref(pred, (9, 5), np.nan_to_num(c["target"]), (9, 7))["total"].backward()
    want = mel_loss_grad_ref(c["pred"], (9, 5), c["target"], (9, 7))
    assert torch.equal(want, pred.grad) and bool((want[torch.from_numpy(c["planted"])] == 0).all())
    mags = want[want != 0].abs().unique()
    assert len(mags) == 1 and abs(float(mags[0]) - 1.0 / (sum(c["n"]) * 8)) <= 1e-18


def test_no_frames_gives_exact_zeros():
    c = mel_case(2, 5, 6, 4, (0, 3), (4, 0))
    ref = mel_loss_ref(c["pred"], (0, 3), c["target"], (4, 0), (0.8, 0.6))
    assert ref["frames"] == 0 and all(float(ref[k]) == 0.0 for k in ("mae", "mse", "mel", "total"))
    assert bool((mel_loss_grad_ref(c["pred"], (0, 3), c["target"], (4, 0), (0.8, 0.6), (1, 1, 1, 1)) == 0).all())


# ------------------------------------------------------------------------------------------------ refusals of the C entries
def _call(lib, entry, order, pointers, defaults, kw):
    """an entry point on a host buffer: every case below is refused before a launch, so nothing dereferences it.  A pointer
    argument is None or a byte offset into the buffer."""
    buf = np.zeros(64, dtype=np.int64)
    a = dict(defaults)
    a.update(kw)
    for name in pointers:
        a[name] = None if a[name] is None else buf.ctypes.data + a[name]
    return getattr(lib, entry)(*[a[k] for k in order], None)


HEAD = ("pred", "ld_row_pred", "ld_batch_pred", "target", "ld_row_target", "ld_batch_target", "pred_lens", "target_lens", "B", "T", "Tt", "M",
        "w_mae", "w_mse")
HEAD_DEFAULTS = dict(pred=0, ld_row_pred=16, ld_batch_pred=160, target=0, ld_row_target=16, ld_batch_target=192, pred_lens=0, target_lens=0,
                     B=2, T=10, Tt=12, M=16, w_mae=1.0, w_mse=0.0)
FWD = dict(order=HEAD + ("extra", "out", "frames", "workspace", "workspace_bytes"),
           pointers=("pred", "target", "pred_lens", "target_lens", "extra", "out", "frames", "workspace"),
           defaults=dict(HEAD_DEFAULTS, extra=0, out=0, frames=0, workspace=0, workspace_bytes=16))
BWD = dict(order=HEAD + ("g_mae", "g_mse", "g_mel", "g_total", "dpred"),
           pointers=("pred", "target", "pred_lens", "target_lens", "g_mae", "g_mse", "g_mel", "g_total", "dpred"),
           defaults=dict(HEAD_DEFAULTS, g_mae=0, g_mse=0, g_mel=0, g_total=0, dpred=0))
COMMON = [(dict(B=0), "B must be in [1, 65535] (one grid row per utterance), got 0"), (dict(B=65536), "got 65536"),
          (dict(T=0), "T must be in [1, 2^20] frames, got 0"), (dict(T=(1 << 20) + 1, ld_batch_pred=1 << 25), f"T must be in [1, 2^20] frames, got {(1 << 20) + 1}"),
          (dict(Tt=0), "Tt must be in [1, 2^20] frames, got 0"), (dict(Tt=(1 << 20) + 1), f"Tt must be in [1, 2^20] frames, got {(1 << 20) + 1}"),
          (dict(M=0), "M must be a multiple of 4 in [4, 4096], got 0"), (dict(M=18, ld_row_pred=20, ld_row_target=20), "got 18"),
          (dict(M=4100), "M must be a multiple of 4 in [4, 4096], got 4100"),
          (dict(ld_row_pred=12), "the row stride of pred must be a multiple of 4 and >= M (ld_row 12, M 16)"),
          (dict(ld_row_pred=18), "the row stride of pred must be a multiple of 4 and >= M (ld_row 18, M 16)"),
          (dict(ld_row_target=12), "the row stride of target must be a multiple of 4 and >= M (ld_row 12, M 16)"),
          (dict(ld_batch_pred=156), "the batch stride of pred must be a multiple of 4 and cover an utterance (ld_batch 156, ld_row 16, frames 10, M 16)"),
          (dict(ld_batch_pred=162), "the batch stride of pred must be a multiple of 4 and cover an utterance (ld_batch 162"),
          (dict(ld_batch_target=188), "the batch stride of target must be a multiple of 4 and cover an utterance (ld_batch 188, ld_row 16, frames 12, M 16)"),
          (dict(ld_row_target=32, ld_batch_target=360), "of target must be a multiple of 4 and cover an utterance (ld_batch 360, ld_row 32, frames 12, M 16)"),
          (dict(B=1, ld_batch_pred=-4), "the batch stride of pred"),
          (dict(w_mae=float("nan")), "the weights must be finite, got nan, 0"), (dict(w_mse=float("inf")), "the weights must be finite, got 1, inf"),
          (dict(pred=8), "pred and target must be 16-byte aligned"), (dict(target=4), "pred and target must be 16-byte aligned"),
          (dict(pred_lens=4), "pred_lens and target_lens must be 8-byte aligned"), (dict(target_lens=12), "8-byte aligned")]


def _nulls(spec, optional=()):
    return [(dict([(name, None)]), "null pointer") for name in spec["pointers"] if name not in optional]


REFUSALS = (
    [("ttts_mel_loss_fwd", FWD, kw, needle) for kw, needle in _nulls(FWD, optional=("extra",)) + COMMON + [
        (dict(extra=2), "extra, out and the workspace must be 4-byte aligned"), (dict(out=1), "4-byte aligned"),
        (dict(workspace=2), "4-byte aligned"), (dict(frames=4), "frames must be 8-byte aligned"),
        (dict(workspace_bytes=15), "the workspace holds 15 bytes, ttts_mel_loss_workspace_bytes asks for 16"),
        (dict(T=33, Tt=40, ld_batch_pred=528, ld_batch_target=640, workspace_bytes=16), "the workspace holds 16 bytes, ttts_mel_loss_workspace_bytes asks for 32")]] +
    [("ttts_mel_loss_bwd", BWD, kw, needle) for kw, needle in _nulls(BWD, optional=("g_mae", "g_mse", "g_mel", "g_total")) + COMMON + [
        (dict(g_mae=2), "the upstream gradients must be 4-byte aligned"), (dict(g_mse=1), "4-byte aligned"), (dict(g_mel=3), "4-byte aligned"),
        (dict(g_total=2), "4-byte aligned"), (dict(dpred=8), "dpred must be 16-byte aligned")]])


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_names_its_value_before_any_launch(case):
    from transformertts_amd import _lib
    lib = _lib.load()
    entry, spec, kw, needle = REFUSALS[case]
    rc = _call(lib, entry, spec["order"], spec["pointers"], spec["defaults"], kw)
    assert rc != 0 and needle in _lib.last_error() and entry[5:] in _lib.last_error(), (entry, kw, _lib.last_error())
    with pytest.raises(RuntimeError, match=re.escape(needle)):       # ... and reaches Python through _lib.check
        _lib.check(rc, entry)


# ------------------------------------------------------------------------------------------------ refusals of the Python checks
def _cuda(shape, dtype=torch.float32, **kw):
    """what the checks read of a device tensor, on the CPU: those in front of the launch can be reached without a device"""
    d = dict(shape=tuple(shape), dim=lambda: len(shape), size=lambda i: tuple(shape)[i], is_cuda=True, dtype=dtype, device="cuda:0")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_mel_loss_refuses():
    from transformertts_amd import student
    from transformertts_amd.student import FastSpeech2Loss, mel_loss
    pl, t = torch.tensor([9, 3, 1]), torch.zeros(3, 12, 8)
    for args, needle in (
            ((torch.zeros(12, 8), pl, t, pl), "mel_loss: pred must be (B, T, M), got (12, 8)"),
            ((torch.zeros(3, 0, 8), pl, t, pl), "mel_loss: pred must be (B, T, M), got (3, 0, 8)"),
            ((torch.zeros(3, 12, 8), pl, t, pl), "mel_loss.pred: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu"),
            ((_cuda((3, 12, 8), torch.float64), pl, t, pl), "mel_loss.pred: expected dtype torch.float32, got torch.float64"),
            ((_cuda((3, 12, 6)), pl, t, pl), "mel_loss: M must be a multiple of 4 in [4, 4096], got 6 (pred)"),
            ((_cuda((3, 12, 4100)), pl, t, pl), "mel_loss: M must be a multiple of 4 in [4, 4096], got 4100 (pred)"),
            ((_cuda((3, (1 << 20) + 1, 8)), pl, t, pl), f"mel_loss: pred must hold [1, 2^20] frames, got {(1 << 20) + 1}"),
            ((_cuda((65536, 12, 8)), pl, t, pl), "mel_loss: B must be in [1, 65535], got 65536")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            mel_loss(*args)
    for bad, needle in ((torch.zeros(2, 12, 8), "mel_loss: target must be (3, Tt, 8) like pred, got (2, 12, 8)"),
                        (torch.zeros(3, 12, 4), "mel_loss: target must be (3, Tt, 8) like pred, got (3, 12, 4)"),
                        (torch.zeros(3, 12), "mel_loss: target must be (3, Tt, 8) like pred, got (3, 12)")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            student._target_like(bad, 3, 8, "mel_loss")
    with pytest.raises(ValueError, match=re.escape("mel_loss.target: expected a CUDA/HIP tensor (the HIP path has no CPU fallback), got cpu")):
        student._mels(student._target_like(t, 3, 8, "mel_loss"), "mel_loss", "target")
    for bad in ((1.0,), (1.0, 2.0, 3.0), (1.0, float("nan")), (float("inf"), 0.0), 1.0):
        with pytest.raises(ValueError, match=re.escape("weights must be two finite numbers (mae, mse), got")):
            student._two_weights(bad, "mel_loss")
    with pytest.raises(ValueError, match=re.escape("FastSpeech2Loss: weights must be two finite numbers (mae, mse), got (1.0,)")):
        FastSpeech2Loss(mel_weights=(1.0,))
    with pytest.raises(ValueError, match=re.escape("VarianceLoss: weights must be three finite numbers")):
        FastSpeech2Loss(variance_weights=(1.0, 1.0))
    assert student._two_weights([1, 0.5], "f") == (1.0, 0.5)
    crit = FastSpeech2Loss()
    assert crit.mel_weights == (1.0, 0.0) and crit.variance.weights == (1.0, 1.0, 1.0)
    dev = torch.device("cpu")
    for bad, what in ((0.5, "float"), (torch.zeros(2), "(2,) torch.float32 on cpu"), (torch.zeros((), dtype=torch.float64), "() torch.float64 on cpu"),
                      (torch.zeros(()), "() torch.float32 on cpu")):
        with pytest.raises(ValueError, match=re.escape(f"mel_loss: extra must be one torch.float32 value on cuda:0 (no CPU fallback), got {what}")):
            student._extra(bad, "cuda:0", "mel_loss")
    assert student._extra(None, dev, "mel_loss") is None and student._extra(torch.zeros(1), dev, "mel_loss").shape == ()
    # the stride rule of variance._rows: a view that breaks it is made contiguous, one that keeps it goes through its strides
    wide = torch.zeros(2, 10, 20)
    for view, want in ((wide[:, :, :16], (20, 200)), (wide[:, :7, 4:20], (20, 200)), (wide[:1, :, :8], (20, 200))):
        x, ld_row, ld_batch = student._mels(types.SimpleNamespace(
            shape=view.shape, dim=view.dim, is_cuda=True, dtype=view.dtype, stride=view.stride, data_ptr=view.data_ptr,
            contiguous=view.contiguous), "f", "x")
        assert (ld_row, ld_batch) == want
    broken = wide[:, :, 2:18]                                          # rows that start 8 bytes off a float4
    x, ld_row, ld_batch = student._mels(types.SimpleNamespace(
        shape=broken.shape, dim=broken.dim, is_cuda=True, dtype=broken.dtype, stride=broken.stride, data_ptr=broken.data_ptr,
        contiguous=broken.contiguous), "f", "x")
    assert x.is_contiguous() and (ld_row, ld_batch) == (16, 160)


# ------------------------------------------------------------------------------------------------ the synthetic batch
@pytest.mark.parametrize("ragged", [False, True])
def test_the_synthetic_student_batch(ragged):
    from transformertts_amd.student import BATCH_KEYS
    from transformertts_amd.workload import synth_batch, synth_student_batch
    b = synth_student_batch(6, 12, n_mels=16, n_vocab=20, max_duration=4, ragged=ragged, seed=5)
    assert tuple(sorted(b)) == tuple(sorted(BATCH_KEYS)) and all(not v.is_cuda and v.is_contiguous() for v in b.values())
    pl, ml = b["phoneme_lens"], b["melspec_lens"]
    assert b["phoneme"].shape == (6, 12) == b["durations"].shape == b["pitch"].shape == b["energy"].shape
    assert b["phoneme"].dtype == b["durations"].dtype == pl.dtype == ml.dtype == torch.int64
    assert b["melspec"].dtype == b["pitch"].dtype == b["energy"].dtype == torch.float32
    assert int(pl.max()) == 12 and int(pl[0]) == 12 and bool((pl[:-1] >= pl[1:]).all())        # one utterance at full length
    assert (len(set(pl.tolist())) > 1) == ragged
    assert b["melspec"].shape == (6, int(ml.max()), 16)
    for i in range(6):
        n = int(pl[i])
        assert int(b["durations"][i, :n].sum()) == int(ml[i])
        assert bool((b["durations"][i, :n] >= 1).all()) and bool((b["durations"][i, :n] <= 4).all())
        assert bool((b["phoneme"][i, :n] >= 1).all()) and bool((b["phoneme"][i, :n] < 20).all())
        assert bool((b["pitch"][i, :n] >= 70).all()) and bool((b["pitch"][i, :n] < 500).all())
        assert bool((b["energy"][i, :n] >= 0).all()) and bool((b["energy"][i, :n] < 1).all())
        for k in ("phoneme", "durations", "pitch", "energy"):
            assert bool((b[k][i, n:] == 0).all()), k
        assert bool((b["melspec"][i, int(ml[i]):] == 0).all()) and bool((b["melspec"][i, :int(ml[i])] != 0).any())
    again = synth_student_batch(6, 12, n_mels=16, n_vocab=20, max_duration=4, ragged=ragged, seed=5)
    assert all(torch.equal(b[k], again[k]) for k in b)
    with pytest.raises(ValueError, match="synth_student_batch: B, Tp, n_mels, max_duration must be positive"):
        synth_student_batch(0)
    # synth_batch is as it was: the flagship's batch
    old = synth_batch(2, 10, 33, 16, 30, ragged=True, seed=4)
    assert tuple(old) == ("phoneme", "melspec", "phoneme_lens", "melspec_lens") and old["melspec"].shape == (2, 33, 16)


# ------------------------------------------------------------------------------------------------ the stepper
def test_the_stepper_refuses_another_optimizer_and_names_a_missing_key():
    from transformertts_amd import student
    from transformertts_amd.student import BATCH_KEYS, StudentTrainStep
    from transformertts_amd.step import TrainStep, _step_seed
    m = torch.nn.Linear(4, 4)
    with pytest.raises(TypeError, match=re.escape("StudentTrainStep drives FlatAdam (flat parameter / gradient / moment buffers)")):
        StudentTrainStep(m, torch.optim.Adam(m.parameters()))
    with pytest.raises(TypeError, match="TrainStep drives FlatAdam"):                          # ... as TrainStep does
        TrainStep(None, torch.optim.Adam(m.parameters()), None)
    assert BATCH_KEYS == ("phoneme", "phoneme_lens", "melspec", "melspec_lens", "durations", "pitch", "energy")
    full = {k: torch.zeros(1) for k in BATCH_KEYS}
    dev = torch.device("cpu")
    student._check_batch(full, dev)
    for k in BATCH_KEYS:
        with pytest.raises(KeyError, match=re.escape(f"StudentTrainStep: the batch lacks {k!r} (it needs phoneme, phoneme_lens, melspec")):
            student._check_batch({j: v for j, v in full.items() if j != k}, dev)
    with pytest.raises(KeyError, match=re.escape("the batch lacks 'pitch', 'energy'")):
        student._check_batch({j: v for j, v in full.items() if j not in ("pitch", "energy")}, dev)
    with pytest.raises(ValueError, match=re.escape("batch['phoneme'] must live on the student's HIP device cuda:0 (no CPU fallback), got cpu")):
        student._check_batch(full, torch.device("cuda:0"))
    # the stepper's __call__ checks the batch first, with nothing of the device touched
    step = object.__new__(StudentTrainStep)
    step.device = dev
    with pytest.raises(KeyError, match="the batch lacks 'durations'"):
        step({j: v for j, v in full.items() if j != "durations"})
    src = open(os.path.join(REPO, "transformertts_amd", "student.py")).read()
    assert "from .step import _step_seed" in src and "def _step_seed" not in src             # imported, not copied
    assert student.__dict__.get("_step_seed") is None and callable(_step_seed)
