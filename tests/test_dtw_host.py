"""DTW mel distance (ABI v22, csrc/dtw.hip; transformertts_amd/metrics.py): the entry points are declared, bound and exported,
ctypes and the header agree, every refusal comes with its message before any launch, the workspace query and its formula, the
argument refusals of `dtw_distance` / `evaluate_synthesis` / `mel_cepstra`, the DCT basis, and the numpy reference the GPU tests
use against a brute-force enumeration of all warping paths.  Host logic only, no GPU."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from dtw_reference import all_paths, brute_force, cell_costs, dtw_from_costs, dtw_ref, path_cost

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_dtw_workspace_bytes", "ttts_dtw")


def test_abi_version_and_the_header_declares_the_new_entry_points():
    from transformertts_amd import _lib, metrics
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 22
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        decl = re.search(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name      # ctypes and the header agree on the argument count
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[NEW[0]] == (Z, [I, I, I])
    assert _lib.SIGNATURES[NEW[1]] == (I, [P, L, L, P, P, L, L, P, I, I, I, I, I, P, Z, P, P, P, P, P, P])
    # the block states what it replaces and the definitions
    block = hdr[hdr.index("ABI v22; dtw.hip"):hdr.index("size_t ttts_dtw_workspace_bytes")]
    for needle in ("torch.cdist", "torch.minimum", "anti-diagonals",
                   "D[0][0] = c[0][0]", "D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1])", "+inf",
                   "the FIRST minimum wins in the order diagonal (i-1, j-1), then (i-1, j), then (i, j-1)",
                   "c[i][j] = sum_k |x[i][k] - y[j][k]|", "c[i][j] = sqrtf(sum_k (x[i][k] - y[j][k])^2)",
                   "cost / (path_len * C) for L1, cost / path_len for L2", "n_b > 0 && m_b > 0",
                   "B * 4 * (Tx * Ty + S * (Tx + 63) * 64 + S * Tx + 2 * (Tx + Ty))"):
        assert needle in block, needle
    assert [int(re.search(rf"#define TTTS_DTW_{m} (\d+)", hdr).group(1)) for m in ("L1", "L2")] == [0, 1]
    assert metrics.METRICS == {"l1": 0, "l2": 1}
    src = open(os.path.join(REPO, "transformertts_amd", "csrc", "dtw.hip")).read()
    assert "the FIRST minimum wins in the order diagonal (i-1, j-1), then (i-1, j), then (i, j-1)" in src
    assert metrics.MAX_LEN == int(re.search(r"DTW_MAX_LEN = (\d+)", src).group(1)) == 4096


def test_entry_point_refuses_bad_arguments_with_a_message():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a2 = ctypes.c_void_p(a.value + 2)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    names = ["x", "ldx_row", "ldx_batch", "x_lens", "y", "ldy_row", "ldy_batch", "y_lens", "B", "Tx", "Ty", "C", "metric", "ws",
             "ws_bytes", "cost", "path_len", "distance", "valid", "path", "stream"]
    need = lib.ttts_dtw_workspace_bytes(2, 7, 5)
    defaults = dict(x=a, ldx_row=13, ldx_batch=91, x_lens=a, y=a, ldy_row=13, ldy_batch=65, y_lens=a, B=2, Tx=7, Ty=5, C=13, metric=0,
                    ws=a, ws_bytes=need, cost=a, path_len=a, distance=a, valid=a, path=None, stream=None)

    def dtw(**kw):
        assert not set(kw) - set(names)
        return lib.ttts_dtw(*[kw.get(n, defaults[n]) for n in names])

    e = "dtw"
    for p in ("x", "x_lens", "y", "y_lens", "ws", "cost", "path_len", "distance", "valid"):
        bad(dtw(**{p: None}), e + ": null pointer")
    bad(dtw(B=0), e + ": sizes must be positive (B 0, Tx 7, Ty 5, C 13)")
    bad(dtw(Tx=-1), e + ": sizes must be positive (B 2, Tx -1, Ty 5, C 13)")
    bad(dtw(Ty=0), e + ": sizes must be positive (B 2, Tx 7, Ty 0, C 13)")
    bad(dtw(C=0, ldx_row=0, ldy_row=0), e + ": sizes must be positive (B 2, Tx 7, Ty 5, C 0)")
    bad(dtw(ldx_row=12), e + ": the row strides must be >= C (ldx_row 12, ldy_row 13, C 13)")
    bad(dtw(ldy_row=1), e + ": the row strides must be >= C (ldx_row 13, ldy_row 1, C 13)")
    bad(dtw(ldx_batch=-91), e + ": strides must not be negative (ldx_batch -91, ldy_batch 65)")
    bad(dtw(ldy_batch=-1), e + ": strides must not be negative (ldx_batch 91, ldy_batch -1)")
    bad(dtw(metric=2), e + ": unknown metric 2")
    bad(dtw(metric=-1), e + ": unknown metric -1")
    bad(dtw(Tx=4097, ws_bytes=1 << 40), e + ": lengths above 4096 frames are not supported (Tx 4097, Ty 5)")
    bad(dtw(Ty=4097, ws_bytes=1 << 40), e + ": lengths above 4096 frames are not supported (Tx 7, Ty 4097)")
    bad(dtw(B=65536, ws_bytes=1 << 40), e + ": grid too large (B 65536, at most 65535 utterances a call)")
    bad(dtw(ws=a2), e + ": the workspace must be 4-byte aligned")
    bad(dtw(ws_bytes=need - 1), e + f": workspace too small ({need - 1} bytes, {need} needed)")
    bad(dtw(ws_bytes=0), e + f": workspace too small (0 bytes, {need} needed)")


def _formula(B, Tx, Ty):
    """the header's: B * 4 * (Tx * Ty + S * (Tx + 63) * 64 + S * Tx + 2 * (Tx + Ty))"""
    K = next((k for k in (1, 2, 4, 8, 16) if 64 * k >= Ty), 16)
    S = -(-Ty // (64 * K))
    return B * 4 * (Tx * Ty + S * (Tx + 63) * 64 + S * Tx + 2 * (Tx + Ty))


def test_workspace_query_matches_the_header_formula_and_is_monotone():
    from transformertts_amd import _lib, metrics
    q = _lib.load().ttts_dtw_workspace_bytes
    assert q(1, 1, 1) == 4 * (1 + 64 * 64 + 1 + 4)
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (1, 4097, 5), (1, 5, 4097)):
        assert q(*bad) == 0
    sizes = (1, 2, 63, 64, 65, 128, 129, 257, 512, 513, 870, 1024, 1025, 2048, 2049, 3072, 3073, 4095)
    for B, Tx, Ty in itertools.product((1, 2, 5, 16), sizes, sizes):
        v = q(B, Tx, Ty)
        assert v == _formula(B, Tx, Ty) and v % 4 == 0
        assert q(B + 1, Tx, Ty) > v and q(B, Tx + 1, Ty) > v and q(B, Tx, Ty + 1) > v
    # 2 bits a cell (over the strips' extent), the staged costs and O(Tx + Ty) at the largest size; a cap of 256 MB holds three such
    top = q(1, 4096, 4096)
    assert top == 4 * 4096 * 4096 + (4096 + 63) * 4096 // 4 + 4 * 4 * 4096 + 8 * 8192 and 3 * top < metrics.WORKSPACE_CAP < 4 * top
    assert metrics.group_size(16, 4096, 4096) == 3 and metrics.group_size(16, 870, 870) == 16
    assert metrics.group_size(16, 870, 870, workspace_cap=1) == 1                        # one utterance at the least
    assert metrics.group_size(10 ** 6, 1, 1, workspace_cap=1 << 40) == 65535


def test_dtw_distance_refuses_bad_arguments():
    import transformertts_amd
    from transformertts_amd.metrics import dtw_distance, evaluate_synthesis, mel_cepstra
    assert transformertts_amd.dtw_distance is dtw_distance and transformertts_amd.evaluate_synthesis is evaluate_synthesis
    assert transformertts_amd.mel_cepstra is mel_cepstra
    x, y, xl, yl = torch.zeros(2, 7, 5), torch.zeros(2, 6, 5), torch.tensor([7, 3]), torch.tensor([6, 4])
    with pytest.raises(ValueError, match="metric must be one of \\('l1', 'l2'\\), got 'cosine'"):
        dtw_distance(x, xl, y, yl, metric="cosine")
    with pytest.raises(ValueError, match="workspace_cap must be a positive number of bytes"):
        dtw_distance(x, xl, y, yl, workspace_cap=0)
    with pytest.raises(ValueError, match="x must be \\(B, T, C\\), got \\(7, 5\\)"):
        dtw_distance(x[0], xl, y, yl)
    with pytest.raises(ValueError, match="empty y \\(2, 0, 5\\)"):
        dtw_distance(x, xl, y[:, :0], yl)
    with pytest.raises(ValueError, match="x and y differ in batch or channels"):
        dtw_distance(x, xl, y[..., :4], yl)
    with pytest.raises(ValueError, match="x and y differ in batch or channels"):
        dtw_distance(x, xl, y[:1], yl)
    with pytest.raises(ValueError, match="y has 4097 frames, above the 4096 the kernels take"):
        dtw_distance(x, xl, torch.zeros(2, 4097, 5), yl)
    with pytest.raises(ValueError, match="x_lens must have shape \\(2,\\), got \\(3,\\)"):
        dtw_distance(x, torch.tensor([1, 2, 3]), y, yl)
    with pytest.raises(ValueError, match="y_lens must be integers"):
        dtw_distance(x, xl, y, yl.float())
    for metric in ("l1", "l2"):
        with pytest.raises(ValueError, match="no CPU fallback"):         # HIP tensors only
            dtw_distance(x, xl, y, yl, metric=metric, path=True)
    with pytest.raises(ValueError, match="dtw_distance.x: expected a CUDA/HIP tensor"):
        dtw_distance(x.double(), xl, y, yl)                             # the device comes before the dtype

    ph, pl = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([4, 2])

    class NeverCalled:
        def synthesize(self, *a, **k):
            raise AssertionError("the refusals come before the synthesis")
    with pytest.raises(ValueError, match="which must be 'post_melspec' or 'pred_melspec', got 'stop'"):
        evaluate_synthesis(NeverCalled(), ph, pl, x, xl, which="stop")
    with pytest.raises(ValueError, match="evaluate_synthesis: metric must be one of"):
        evaluate_synthesis(NeverCalled(), ph, pl, x, xl, metric="dtw")
    with pytest.raises(ValueError, match="melspec must be \\(B, T, n_mels\\)"):
        evaluate_synthesis(NeverCalled(), ph, pl, x[0], xl)
    with pytest.raises(ValueError, match="phoneme must be \\(B, Tp\\) = \\(2, Tp\\)"):
        evaluate_synthesis(NeverCalled(), ph[:1], pl, x, xl)
    with pytest.raises(ValueError, match="melspec_lens must have shape \\(2,\\)"):
        evaluate_synthesis(NeverCalled(), ph, pl, x, xl[:1])
    with pytest.raises(ValueError, match="melspec_lens must be integers"):
        evaluate_synthesis(NeverCalled(), ph, pl, x, xl.float())

    with pytest.raises(ValueError, match="n_coef must be an integer in \\[1, n_mels = 5\\)"):
        mel_cepstra(x, n_coef=5)
    with pytest.raises(ValueError, match="give both `mean` and `std`"):
        mel_cepstra(x, n_coef=3, mean=torch.zeros(5))
    with pytest.raises(ValueError, match="no CPU fallback"):
        mel_cepstra(x, n_coef=3)


def test_which_operand_layouts_are_read_in_place():
    from transformertts_amd.metrics import _strides
    B, T, C = 3, 5, 7
    assert _strides(torch.zeros(B, T, C)) == (C, T * C)
    assert _strides(torch.zeros(B, T, C + 3)[..., :C]) == (C + 3, T * (C + 3))               # padded rows: a view, in place
    assert _strides(torch.zeros(B + 2, T, C)[1:4]) == (C, T * C)                             # a sliced batch
    assert _strides(torch.zeros(B, T, 12)[..., 1:8]) == (12, T * 12)                         # no alignment is asked
    assert _strides(torch.zeros(1, T, C).expand(B, T, C)) == (C, 0)
    assert _strides(torch.zeros(B, C, T).transpose(1, 2)) is None                            # channels not contiguous
    assert _strides(torch.zeros(B, T, 2 * C)[..., ::2]) is None
    assert _strides(torch.zeros(1, 1, C)) == (C, 0)


def test_the_numpy_reference_against_every_warping_path():
    """for every (n, m) with n, m <= 5: integer costs, so the recurrence's cost equals the least cost over all enumerated paths
    exactly, in fp32 and in fp64; the returned path is a warping path of that cost and obeys the tie rule at every cell"""
    rng = np.random.default_rng(5)
    assert len(all_paths(5, 5)) == 321 and len(all_paths(1, 4)) == 1 and len(all_paths(2, 2)) == 3   # (Delannoy numbers)
    for n, m in itertools.product(range(1, 6), repeat=2):
        for trial in range(4):
            C = (1, 3)[trial % 2]
            x, y = rng.integers(-3, 4, (n, C)), rng.integers(-3, 4, (m, C))
            c64 = cell_costs(x, y, "l1", np.float64)
            assert np.array_equal(c64, np.abs(x[:, None] - y[None]).sum(-1))
            best = brute_force(c64)
            for dtype in (np.float32, np.float64):
                cost, path = dtw_ref(x, y, "l1", dtype)
                assert cost.dtype == dtype and float(cost) == float(best), (n, m)
                assert path[0] == (0, 0) and path[-1] == (n - 1, m - 1)
                assert all((b[0] - a[0], b[1] - a[1]) in ((1, 0), (0, 1), (1, 1)) for a, b in zip(path, path[1:]))
                assert path_cost(c64, path) == best
    # ties everywhere: the diagonal wins, then (i-1, j), then (i, j-1)
    assert dtw_from_costs(np.zeros((3, 3), np.float32))[1] == [(0, 0), (1, 1), (2, 2)]
    assert dtw_from_costs(np.zeros((2, 3), np.float32))[1] == [(0, 0), (0, 1), (1, 2)]
    assert dtw_from_costs(np.zeros((3, 2), np.float32))[1] == [(0, 0), (1, 0), (2, 1)]
    up_or_left = np.array([[0, 0], [0, 5], ], np.float32)                 # (1,1): diagonal 0 = up 0 = left 0 -> diagonal
    assert dtw_from_costs(up_or_left)[1] == [(0, 0), (1, 1)]
    c = np.array([[1, 0], [0, 0]], np.float32)                            # D = [[1, 1], [1, .]]: all three equal -> diagonal
    assert dtw_from_costs(c)[1] == [(0, 0), (1, 1)]
    c = np.array([[0, 0, 0], [9, 9, 0]], np.float64)                      # up (0,2) = 0 beats the diagonal (0,1) = 0?  no: diagonal first
    assert dtw_from_costs(c)[1] == [(0, 0), (0, 1), (1, 2)]
    c = np.array([[0, 5], [0, 0]], np.float64)                            # at (1,1): diagonal 0, up 5, left 0 -> diagonal
    assert dtw_from_costs(c)[1] == [(0, 0), (1, 1)]
    c = np.array([[3, 0], [0, 0]], np.float64)                            # at (1,1): diagonal 3, up 3, left 3 -> diagonal
    assert dtw_from_costs(c) == (3.0, [(0, 0), (1, 1)])
    c = np.array([[3, -1], [-1, 0]], np.float64)                          # diagonal 3, up 2, left 2 -> (i-1, j)
    assert dtw_from_costs(c) == (2.0, [(0, 0), (0, 1), (1, 1)])
    # the l2 cost is the Euclidean distance, and fp32 / fp64 agree to rounding
    x, y = rng.standard_normal((6, 13)), rng.standard_normal((4, 13))
    c64 = cell_costs(x, y, "l2", np.float64)
    assert np.allclose(c64, np.sqrt(((x[:, None] - y[None]) ** 2).sum(-1)), rtol=1e-14)
    assert np.allclose(cell_costs(x, y, "l2", np.float32), c64, rtol=1e-5)


def test_the_dct_basis_is_orthonormal_and_is_the_dct_ii():
    from transformertts_amd.metrics import dct_basis
    for n_mels, n_coef in ((80, 13), (80, 79), (20, 5), (8, 7)):
        k, c = np.arange(n_mels)[None, :], np.arange(1, n_coef + 1)[:, None]
        want = np.sqrt(2.0 / n_mels) * np.cos(np.pi * (2 * k + 1) * c / (2 * n_mels))         # DCT-II, norm="ortho", rows 1 .. n_coef
        got = dct_basis(n_mels, n_coef, dtype=torch.float64).numpy()
        assert got.shape == (n_coef, n_mels) and np.abs(got - want).max() < 1e-12
        assert np.abs(got @ got.T - np.eye(n_coef)).max() < 1e-12                             # orthonormal rows
        assert np.abs(got.sum(1)).max() < 1e-12                                               # ... orthogonal to the dropped row 0
    assert dct_basis(80, 13).dtype == torch.float32
    assert abs(10 * math.sqrt(2) / math.log(10) - 6.141851463713754) < 1e-12                  # the MCD factor of the docstring


def test_the_module_reads_the_free_running_key():
    """construction only (no device): absent or None leaves the module without the free-running pass"""
    from oracle import model_config
    from transformertts_amd.lightning_module import LightningModule
    training = {"num_epochs": 3, "teacher_forcing_mode": "linear", "warmup_steps": 5}
    mk = lambda t: LightningModule({"model": dict(model_config("micro"), device="cpu"), "loss": {"stop_weight": 8.0}, "training": t})
    assert mk(training).free_running is None and mk(dict(training, free_running_validation=None)).free_running is None
    lm = mk(dict(training, free_running_validation={"utterances": 2, "max_len": 30}))
    assert lm.free_running == {"utterances": 2, "max_len": 30} and lm._synthesizer is None
    lm.valid_losses.append(1.5)
    lm2 = mk(training)
    lm2.valid_losses.append(1.5)
    lm2.on_validation_epoch_end()
    assert lm2._logged == {"val_loss": 1.5}
    lm.on_validation_epoch_end()                                          # no example batch yet: nothing to synthesise
    assert lm._logged == {"val_loss": 1.5}


def test_the_benchmarks_stock_torch_side_is_the_same_computation():
    """tools/dtw_bench.py times the kernels against `torch_dtw`; on CPU tensors with integer features (every sum exact) it gives
    the cost and the path length of the sequential reference, zero-length and clamped rows included"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import dtw_bench as bench
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(9)
    lens = [(1, 1), (1, 7), (7, 1), (12, 9), (0, 5), (5, 0), (9, 12), (30, 20)]
    Tx, Ty, C = 12, 12, 3
    x, y = rng.integers(-3, 4, (len(lens), Tx, C)), rng.integers(-3, 4, (len(lens), Ty, C))
    xl, yl = torch.tensor([l[0] for l in lens]), torch.tensor([l[1] for l in lens])
    cost, plen = bench.torch_dtw(torch.from_numpy(x).float(), xl, torch.from_numpy(y).float(), yl)
    for b, (n, m) in enumerate(lens):
        n, m = min(n, Tx), min(m, Ty)
        if n == 0 or m == 0:
            assert float(cost[b]) == 0.0 and int(plen[b]) == 0
            continue
        want, path = dtw_ref(x[b, :n], y[b, :m], "l1", np.float32)
        assert float(cost[b]) == float(want) and int(plen[b]) == len(path), (n, m)
    assert [c[1:4] for c in bench.CONFIGS] == [(1, 870, 870), (16, 870, 870), (16, 1499, 1499)] and bench.CONFIGS[2][4] == (300, 1499)
    xs, xls, ys, yls = bench.make_case(16, 1499, 1499, 80, "cpu", (300, 1499))
    assert int(xls.min()) >= 300 and int(yls.min()) >= 300 and int(xls[0]) == int(yls[0]) == 1499 and tuple(xs.shape) == (16, 1499, 80)
