"""DTW mel distance on the GPU (csrc/dtw.hip, transformertts_amd/metrics.py, ABI v22): the kernels against the sequential numpy
references of tests/dtw_reference.py -- bit for bit on integer features, within the rounding bound on normal ones -- the path's
properties, the identities, reads and writes inside the lengths, batch and group independence, repeatability and graph capture,
`evaluate_synthesis` on the tiny model and the free-running validation of the LightningModule."""
import functools

import numpy as np
import pytest
import torch

from conftest import guarded
from dtw_reference import cell_costs, dtw_from_costs, path_cost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = ((1, 1), (1, 7), (7, 1), (63, 65), (64, 64), (65, 63), (129, 40), (40, 129), (200, 257))
# beyond the listed pairs: more than one strip of 1024 columns (the edge hand-over and a backtrack that crosses strips)
WIDE = (70, 1100)


@functools.lru_cache(maxsize=None)
def _ints(n, m, C):
    """integer features in [-3, 3] and the sequential fp32 reference (every cost and partial sum is exact; ties everywhere)"""
    rng = np.random.default_rng(1000 * n + 7 * m + C)
    x, y = rng.integers(-3, 4, (n, C)).astype(np.float32), rng.integers(-3, 4, (m, C)).astype(np.float32)
    cost, path = dtw_from_costs(cell_costs(x, y, "l1", np.float32))
    return x, y, cost, path


@functools.lru_cache(maxsize=None)
def _normals(n, m, C, metric):
    """standard-normal features and the fp64 reference -> (x, y, c64, cost64)"""
    rng = np.random.default_rng(2000 * n + 11 * m + C)
    x, y = rng.standard_normal((n, C)).astype(np.float32), rng.standard_normal((m, C)).astype(np.float32)
    c64 = cell_costs(x, y, metric, np.float64)
    return x, y, c64, float(dtw_from_costs(c64)[0])


def _batch(rows, Tx=None, Ty=None, fill=0.0):
    """rows of (x (n, C), y (m, C)) -> x (B, Tx, C), x_lens, y (B, Ty, C), y_lens on the device, `fill` behind the lengths"""
    C = rows[0][0].shape[1]
    Tx = Tx or max(max(r[0].shape[0] for r in rows), 1)
    Ty = Ty or max(max(r[1].shape[0] for r in rows), 1)
    x, y = torch.full((len(rows), Tx, C), fill), torch.full((len(rows), Ty, C), fill)
    for b, (xr, yr) in enumerate(rows):
        x[b, :xr.shape[0]] = torch.from_numpy(xr)
        y[b, :yr.shape[0]] = torch.from_numpy(yr)
    lens = lambda i: torch.tensor([r[i].shape[0] for r in rows])
    return x.to(DEV), lens(0).to(DEV), y.to(DEV), lens(1).to(DEV)


def _paths(out):
    """the returned paths as lists of (i, j), after checking the -1 fill and path_len against them"""
    cells, plen = out["path"].cpu(), out["path_len"].cpu()
    res = []
    for b in range(cells.size(0)):
        k = int(plen[b])
        assert bool((cells[b, k:] == -1).all()) and bool((cells[b, :k] >= 0).all())
        res.append([tuple(c) for c in cells[b, :k].tolist()])
    return res


def _check_path(path, n, m):
    assert path[0] == (0, 0) and path[-1] == (n - 1, m - 1)
    assert all((b[0] - a[0], b[1] - a[1]) in ((1, 0), (0, 1), (1, 1)) for a, b in zip(path, path[1:]))
    assert max(n, m) <= len(path) <= n + m - 1


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ================================================================================================ 1. exact on integers
@pytest.mark.parametrize("C", [1, 13, 80])
def test_integer_features_match_the_sequential_reference_bit_for_bit(C):
    from transformertts_amd import dtw_distance
    pairs = PAIRS + ((WIDE,) if C == 1 else ())
    for n, m in pairs:                                                    # each pair at its own extents: every column count per lane
        x, y, cost, path = _ints(n, m, C)
        out = dtw_distance(*_batch([(x, y)]), metric="l1", path=True)
        assert tuple(out["path"].shape) == (1, n + m - 1, 2) and out["path"].dtype == torch.int32
        assert float(out["cost"][0]) == float(cost) and int(out["path_len"][0]) == len(path), (n, m)
        assert _paths(out)[0] == path, (n, m)
        _check_path(path, n, m)
        assert float(out["distance"][0]) == float(np.float32(cost) / (np.float32(len(path)) * np.float32(C)))
        assert bool(out["valid"][0]) and out["valid"].dtype == torch.bool and out["path_len"].dtype == torch.int64
    rows = [_ints(n, m, C)[:2] for n, m in PAIRS]                         # ... and all of them as rows of one padded batch
    out = dtw_distance(*_batch(rows), metric="l1", path=True)
    got = _paths(out)
    for b, (n, m) in enumerate(PAIRS):
        _, _, cost, path = _ints(n, m, C)
        assert float(out["cost"][b]) == float(cost) and got[b] == path, (n, m)


def test_ragged_rows_under_extents_of_more_than_one_strip():
    """16 columns a lane and two strips by the extents, rows that use one strip or both, that end on a strip's last column and
    on the first of the next"""
    from transformertts_amd import dtw_distance
    pairs = (WIDE, (30, 500), (25, 1050), (9, 1024), (33, 1025))
    out = dtw_distance(*_batch([_ints(n, m, 1)[:2] for n, m in pairs], fill=float("nan")), metric="l1", path=True)
    got = _paths(out)
    for b, (n, m) in enumerate(pairs):
        _, _, cost, path = _ints(n, m, 1)
        assert float(out["cost"][b]) == float(cost) and got[b] == path, (n, m)


def test_a_ragged_batch_with_zero_lengths():
    from transformertts_amd import dtw_distance
    C = 13
    empty = np.zeros((0, C), np.float32)
    rows = [_ints(40, 129, C)[:2], (empty, _ints(7, 1, C)[1]), _ints(65, 63, C)[:2], (_ints(7, 1, C)[0], empty), (empty, empty)]
    x, xl, y, yl = _batch(rows, fill=float("nan"))
    for metric in ("l2", "l1"):
        out = dtw_distance(x, xl, y, yl, metric=metric, path=True)
        assert out["valid"].tolist() == [True, False, True, False, False]
        got = _paths(out)
        for b in (1, 3, 4):
            assert float(out["cost"][b]) == 0.0 and float(out["distance"][b]) == 0.0 and int(out["path_len"][b]) == 0 and got[b] == []
            assert bool((out["path"][b] == -1).all())
        for b, (n, m) in ((0, (40, 129)), (2, (65, 63))):
            _check_path(got[b], n, m)
            if metric == "l1":
                assert float(out["cost"][b]) == float(_ints(n, m, C)[2]) and got[b] == _ints(n, m, C)[3]
    # lengths beyond the extents are clamped to them, negative ones to 0 (`out` is the l1 result)
    out2 = dtw_distance(x, xl + torch.tensor([1000, -5, 0, 0, 0], device=DEV), y, yl, metric="l1", path=True)
    assert out2["valid"].tolist() == [True, False, True, False, False] and torch.equal(out2["path"][2], out["path"][2])


# ================================================================================================ 2. normal features
@pytest.mark.parametrize("metric", ["l1", "l2"])
def test_normal_features_are_within_the_rounding_bound_of_the_fp64_reference(metric):
    """eps = (Tx + Ty + C) 2^-24: all terms are non-negative, an fp32 sum of n of them is off by at most n 2^-24 relative, a cell
    cost by about (C + 1) 2^-24, min is exact.  |cost - cost64| <= 2 eps cost64, and the returned path, re-evaluated in fp64,
    costs at most (1 + 4 eps) times the fp64 optimum (2 and 4: second-order terms and the square root's rounding)."""
    from transformertts_amd import dtw_distance
    cases = [(n, m, 80) for n, m in PAIRS] + [(300, 280, 13)]
    for C in (80, 13):
        these = [c for c in cases if c[2] == C]
        rows = [_normals(n, m, C, metric)[:2] for n, m, _ in these]
        out = dtw_distance(*_batch(rows), metric=metric, path=True)
        got = _paths(out)
        for b, (n, m, _) in enumerate(these):
            _, _, c64, cost64 = _normals(n, m, C, metric)
            eps = (n + m + C) * 2.0 ** -24
            cost = float(out["cost"][b])
            print(f"{metric} ({n}, {m}, C {C}): |cost - cost64| / cost64 = {abs(cost - cost64) / cost64:.3e} (bound {2 * eps:.3e}), "
                  f"path cost / optimum - 1 = {path_cost(c64, got[b]) / cost64 - 1:.3e} (bound {4 * eps:.3e})")
            assert abs(cost - cost64) <= 2 * eps * cost64, (n, m)
            _check_path(got[b], n, m)
            assert path_cost(c64, got[b]) <= (1 + 4 * eps) * cost64, (n, m)
            norm = len(got[b]) * (C if metric == "l1" else 1)
            assert abs(float(out["distance"][b]) - cost64 / norm) <= 3 * eps * cost64 / norm


# ================================================================================================ 3. identities
@pytest.mark.parametrize("metric", ["l1", "l2"])
def test_identities(metric):
    from transformertts_amd import dtw_distance
    rows = [(_normals(n, 1, 13, "l1")[0],) * 2 for n in (1, 63, 129, 200)]
    x, xl, _, _ = _batch(rows)
    out = dtw_distance(x, xl, x, xl, metric=metric, path=True)           # dtw(x, x): the diagonal, at no cost
    assert out["cost"].tolist() == [0.0] * 4 and torch.equal(out["path_len"], xl) and out["distance"].tolist() == [0.0] * 4
    for b, p in enumerate(_paths(out)):
        assert p == [(i, i) for i in range(int(xl[b]))]
    y = x.repeat_interleave(2, dim=1)                                     # every frame twice: still no cost, two cells a frame
    out = dtw_distance(x, xl, y, 2 * xl, metric=metric, path=True)
    assert out["cost"].tolist() == [0.0] * 4 and torch.equal(out["path_len"], 2 * xl)
    for b, p in enumerate(_paths(out)):
        _check_path(p, int(xl[b]), 2 * int(xl[b]))
        assert all(j // 2 == i for i, j in p)


def test_the_largest_lengths():
    """4096 frames a side: four strips of 1024 columns, 71.5 MB of workspace an utterance.  No reference runs at this size in a
    test's time, so: the identity, and on integer features a path with every property whose own cost -- exact in fp32 -- is the
    cost the recurrence returns (optimality is what the smaller sizes check)."""
    from transformertts_amd import dtw_distance
    rng = np.random.default_rng(4096)
    x, y = rng.integers(-3, 4, (4096, 1)).astype(np.float32), rng.integers(-3, 4, (4000, 1)).astype(np.float32)
    xd, xl, yd, yl = _batch([(x, x), (x, y)], fill=float("nan"))
    out = dtw_distance(xd, xl, yd, yl, metric="l1", path=True)
    got = _paths(out)
    assert float(out["cost"][0]) == 0.0 and got[0] == [(i, i) for i in range(4096)]
    _check_path(got[1], 4096, 4000)
    i, j = np.array(got[1]).T
    assert float(out["cost"][1]) == float(np.abs(x[i, 0] - y[j, 0]).sum(dtype=np.float64)) > 0
    with pytest.raises(ValueError, match="x has 4097 frames"):
        dtw_distance(torch.zeros(1, 4097, 1, device=DEV), xl[:1], yd[:1], yl[:1])


# ================================================================================================ 4. inside the lengths
def test_nothing_is_read_or_written_past_the_lengths():
    from transformertts_amd import _lib, metrics
    C, B = 13, 4
    rows = [_normals(n, m, C, "l1")[:2] for n, m in ((63, 65), (129, 40), (7, 1), (40, 129))]
    tight = _batch(rows)
    Tx, Ty = tight[0].size(1), tight[2].size(1)
    want = metrics.dtw_distance(*tight, metric="l2", path=True)
    # NaN at and behind every length, rows of C + 3 floats, a sliced batch dimension
    bx, by = torch.full((B + 2, Tx + 1, C + 3), float("nan"), device=DEV), torch.full((B + 3, Ty + 2, C + 3), float("nan"), device=DEV)
    xv, yv = bx[1:B + 1, :Tx, 2:C + 2], by[2:B + 2, :Ty, :C]
    for b, (xr, yr) in enumerate(rows):
        xv[b, :xr.shape[0]] = torch.from_numpy(xr).to(DEV)
        yv[b, :yr.shape[0]] = torch.from_numpy(yr).to(DEV)
    assert metrics._strides(xv) == (C + 3, (Tx + 1) * (C + 3)) and not xv.is_contiguous()
    _same(metrics.dtw_distance(xv, tight[1], yv, tight[3], metric="l2", path=True), want)
    # outputs and workspace with sentinel rows behind them
    words = _lib.load().ttts_dtw_workspace_bytes(B, Tx, Ty) // 4
    arrays = {"ws": guarded((words, 1), 0.0), "cost": guarded((B, 1), 0.0), "path_len": guarded((B, 2), 0.0),
              "distance": guarded((B, 1), 0.0), "valid": guarded((1, 1), 0.0), "path": guarded((B, (Tx + Ty - 1) * 2), 0.0)}
    assert B == 4                                                         # (B bytes of `valid` fill the one guarded float)
    view = {"ws": arrays["ws"][0], "cost": arrays["cost"][0], "path_len": arrays["path_len"][0].view(torch.int64),
            "distance": arrays["distance"][0], "valid": arrays["valid"][0].view(torch.uint8), "path": arrays["path"][0].view(torch.int32)}
    metrics._dtw_into(xv, tight[1], yv, tight[3], metrics.METRICS["l2"], view["ws"], view["cost"], view["path_len"], view["distance"],
                      view["valid"], view["path"])
    torch.cuda.synchronize()
    for name, (_, check) in arrays.items():
        check()
    assert torch.equal(view["cost"].view(B), want["cost"]) and torch.equal(view["path_len"].view(B), want["path_len"])
    assert torch.equal(view["distance"].view(B), want["distance"]) and view["valid"].view(B).tolist() == [1] * B
    assert torch.equal(view["path"].view(B, Tx + Ty - 1, 2), want["path"])


# ================================================================================================ 5. batch independence
def test_rows_and_groups_are_independent():
    from transformertts_amd import dtw_distance, metrics
    C = 80
    rows = [_normals(n, m, C, "l1")[:2] for n, m in ((200, 257), (1, 7), (64, 64), (129, 40), (65, 63))]
    x, xl, y, yl = _batch(rows, fill=float("nan"))
    for metric in ("l1", "l2"):
        whole = dtw_distance(x, xl, y, yl, metric=metric, path=True)
        for b, (xr, yr) in enumerate(rows):                               # row b alone, at its own extents
            one = dtw_distance(*_batch([(xr, yr)]), metric=metric, path=True)
            k = int(one["path_len"][0])
            assert torch.equal(one["cost"][0], whole["cost"][b]) and torch.equal(one["distance"][0], whole["distance"][b])
            assert k == int(whole["path_len"][b]) and torch.equal(one["path"][0, :k], whole["path"][b, :k])
        assert metrics.group_size(5, x.size(1), y.size(1), workspace_cap=1) == 1
        _same(dtw_distance(x, xl, y, yl, metric=metric, path=True, workspace_cap=1), whole)          # five groups of one
        from transformertts_amd import _lib
        per = _lib.load().ttts_dtw_workspace_bytes(1, x.size(1), y.size(1))
        assert metrics.group_size(5, x.size(1), y.size(1), workspace_cap=2 * per + 1) == 2
        _same(dtw_distance(x, xl, y, yl, metric=metric, path=True, workspace_cap=2 * per + 1), whole)  # groups of 2, 2, 1
        _same(dtw_distance(x, xl, y, yl, metric=metric, path=True), whole)                           # two calls, bit for bit
        assert set(dtw_distance(x, xl, y, yl, metric=metric)) == {"cost", "path_len", "distance", "valid"}


# ================================================================================================ 6. graphs
def test_the_call_captures_into_a_graph_and_lengths_are_data():
    from transformertts_amd import dtw_distance
    C = 13
    rows = [_normals(n, m, C, "l1")[:2] for n, m in ((129, 40), (63, 65), (40, 129))]
    x, xl, y, yl = _batch(rows)
    eager = dtw_distance(x, xl, y, yl, metric="l1", path=True)
    xl_s, yl_s = xl.clone(), yl.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = dtw_distance(x, xl_s, y, yl_s, metric="l1", path=True)
    g.replay()
    torch.cuda.synchronize()
    _same({k: v.clone() for k, v in out.items()}, eager)
    new_xl, new_yl = torch.tensor([50, 0, 40], device=DEV), torch.tensor([40, 65, 7], device=DEV)
    xl_s.copy_(new_xl)
    yl_s.copy_(new_yl)
    g.replay()
    torch.cuda.synchronize()
    _same({k: v.clone() for k, v in out.items()}, dtw_distance(x, new_xl, y, new_yl, metric="l1", path=True))
    assert out["valid"].tolist() == [True, False, True]


# ================================================================================================ 7. cepstra
def test_mel_cepstra_is_the_dct_of_the_denormalised_mel():
    from transformertts_amd import dtw_distance, mel_cepstra
    from transformertts_amd.metrics import dct_basis
    g = torch.Generator().manual_seed(3)
    mel, mean, std = torch.randn(2, 37, 80, generator=g), torch.randn(80, generator=g), torch.rand(80, generator=g) + 0.5
    got = mel_cepstra(mel.to(DEV), n_coef=13, mean=mean.to(DEV), std=std.to(DEV))
    want = (mel.double() * (std.double() + 1e-8) + mean.double()) @ dct_basis(80, 13, dtype=torch.float64).T
    assert tuple(got.shape) == (2, 37, 13) and got.dtype == torch.float32
    assert float((got.cpu().double() - want).norm() / want.norm()) < 1e-5
    plain = mel_cepstra(mel.to(DEV))
    assert float((plain.cpu().double() - mel.double() @ dct_basis(80, 13, dtype=torch.float64).T).norm()) < 1e-5 * float(mel.norm())
    lens = torch.tensor([37, 20], device=DEV)
    out = dtw_distance(plain, lens, plain, lens, metric="l2")
    assert out["distance"].tolist() == [0.0, 0.0]


# ================================================================================================ 8. end to end
def _tiny():
    from oracle import synth_batch
    from test_hip_model import _build
    cfg, m = _build("tiny", 11)
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    return cfg, m, batch, [batch[k].to(DEV) for k in ("phoneme", "phoneme_lens", "melspec", "melspec_lens")]


def test_evaluate_synthesis_on_the_tiny_model():
    from transformertts_amd import dtw_distance, evaluate_synthesis
    from transformertts_amd.synthesis import Synthesizer
    cfg, m, batch, (ph, pl, mel, ml) = _tiny()
    synth = Synthesizer(m)
    for kw in (dict(max_len=40, stop_threshold=0.5), dict(max_len=24, stop_threshold=2.0, metric="l2", which="pred_melspec")):
        res = evaluate_synthesis(synth, ph, pl, mel, ml, **kw)
        assert set(res) == {"distance", "cost", "path_len", "valid", "mel_lens", "len_ratio", "unfinished"}
        assert all(v.is_cuda and tuple(v.shape) == (3,) for v in res.values())
        out = synth.synthesize(ph, pl, max_len=kw["max_len"], stop_threshold=kw["stop_threshold"])
        by_hand = dtw_distance(out[kw.get("which", "post_melspec")], out["mel_lens"], mel, ml, metric=kw.get("metric", "l1"))
        for k in ("distance", "cost", "path_len", "valid"):
            assert torch.equal(res[k], by_hand[k]), k
        assert torch.equal(res["mel_lens"], out["mel_lens"]) and bool(res["valid"].all()) and bool((res["distance"] > 0).all())
        assert torch.equal(res["len_ratio"], out["mel_lens"].float() / ml.float()) and res["len_ratio"].dtype == torch.float32
        assert res["unfinished"].dtype == torch.bool and torch.equal(res["unfinished"], out["mel_lens"] == kw["max_len"] - 1)
        if kw["stop_threshold"] > 1.0:                                    # a threshold no sigmoid reaches: every row runs out
            assert res["unfinished"].tolist() == [True] * 3 and res["mel_lens"].tolist() == [kw["max_len"] - 1] * 3
        # the synthesised mels against themselves: no distance; a recording of length 0: ratio 0, not valid
        self_ = evaluate_synthesis(synth, ph, pl, out["post_melspec"], out["mel_lens"], max_len=kw["max_len"],
                                   stop_threshold=kw["stop_threshold"])
        assert self_["distance"].tolist() == [0.0] * 3 and self_["len_ratio"].tolist() == [1.0] * 3
    ml0 = ml.clone()
    ml0[1] = 0
    res = evaluate_synthesis(synth, ph, pl, mel, ml0, max_len=24)
    assert res["valid"].tolist() == [True, False, True] and float(res["len_ratio"][1]) == 0.0 and float(res["distance"][1]) == 0.0


def _module(free_running):
    from oracle import fill_state
    from transformertts_amd.lightning_module import LightningModule
    from transformertts_amd.workload import model_config
    cfg = model_config("tiny")
    training = {"num_epochs": 300, "teacher_forcing_mode": "linear", "warmup_steps": 50}
    if free_running is not None:
        training["free_running_validation"] = free_running
    lm = LightningModule({"model": dict(cfg, device="cuda"), "loss": {"stop_weight": 8.0}, "training": training}).to("cuda")
    lm.model.load_state_dict(fill_state(cfg, 11), strict=True)
    return cfg, lm


def test_the_module_logs_the_free_running_numbers():
    from oracle import synth_batch
    from transformertts_amd import AttentionWindow, evaluate_synthesis
    from transformertts_amd.synthesis import Synthesizer
    window = {"guide": (0, 0), "back": 1, "ahead": 3}
    for fr in ({"utterances": 2, "max_len": 30}, {"utterances": 3, "max_len": 24, "stop_threshold": 2.0, "metric": "l2", "window": window}):
        cfg, lm = _module(fr)
        batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
        lm.eval()
        with torch.no_grad():
            lm.validation_step(batch, 0)
        lm.on_validation_epoch_end()
        assert set(lm._logged) == {"val_loss", "val_free_mel_dtw", "val_free_len_ratio", "val_free_unfinished"}
        assert not lm.training and not any(mod.training for mod in lm.modules())
        n = fr["utterances"]
        args = [batch[k][:n].to(DEV) for k in ("phoneme", "phoneme_lens", "melspec", "melspec_lens")]
        res = evaluate_synthesis(Synthesizer(lm.model), *args, max_len=fr["max_len"], stop_threshold=fr.get("stop_threshold", 0.5),
                                 metric=fr.get("metric", "l1"), window=AttentionWindow(**window) if "window" in fr else None)
        assert bool(res["valid"].all())
        # (means of at most three fp32 values, taken in two orders: equal to a few 2^-24)
        assert lm._logged["val_free_mel_dtw"] == pytest.approx(float(res["distance"].double().mean()), rel=1e-6)
        assert lm._logged["val_free_len_ratio"] == pytest.approx(float(res["len_ratio"].double().mean()), rel=1e-6)
        assert lm._logged["val_free_unfinished"] == pytest.approx(float(res["unfinished"].double().mean()), rel=1e-6)
        if "stop_threshold" in fr:
            assert lm._logged["val_free_unfinished"] == 1.0
        first = lm._synthesizer
        lm.train()
        lm.on_validation_epoch_end()                                      # the next epoch: the same Synthesizer, the flags kept
        assert lm._synthesizer is first and lm.training and all(mod.training for mod in lm.modules())
    cfg, lm = _module(None)
    lm.eval()
    with torch.no_grad():
        lm.validation_step(synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21), 0)
    lm.on_validation_epoch_end()
    assert set(lm._logged) == {"val_loss"} and lm._synthesizer is None
