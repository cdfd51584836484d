"""The convolution kernels at 1, 3, 7 and 9 taps (everything else in the suite runs them at 5): weight gradients in their three
forms and as members of grouped launches, forward and data gradient through the fp16x3 weight image (nine taps: its second pass of
eight), the BatchNorm partials of the forward epilogue, and ops.conv_bn end to end -- against torch's conv1d (padding = taps // 2)
and its autograd in fp64, under conftest.rel_l2 and the TOL of tests/test_hip_modes.py.  Gradient cases scale dy by 2e-7 (what a
mean-reduced loss hands down), so the dynamic pre-scale works.  Every case first asserts, through the library's own queries, the
planner branch it was written for.  Measured errors: parity_reports/conv_taps_margin.txt (as measured on one MI355X:
tests/reports/conv_taps_margin.txt).

What is not reachable, and why:
  * class 2 (whole 256 x 256 tiles by LDS-DMA, wgrad_dma_body) needs at least three tile-taps: at cin = cout = 256 no 1-tap
    problem is of that class (ttts_wgrad_group_ok answers 1); it runs at 3, 7 and 9 taps here.
  * class 2 is a plan of the fp16x3 form alone: ttts_conv1d_bwd_weight / _x6 have no such kernel, so the 25 600-row shapes run on
    the _h3 entry only (the other two forms would repeat, slowly, the tiles the small shapes already cover).
  * the 224-row forward tile needs three k-tiles and 32 769 rows at 256 channels; it runs at 3 and 9 taps (the smallest and the
    two-pass image), not at every count.
  * a convolution of ONE tap in a grouped launch is a linear member (taps = 1, T = 0): the group has no other form for it."""
import ctypes
import os

import pytest
import torch

from test_hip_dropout_parity import REPORT_DIR
from test_hip_modes import (TOL, _bn_statistics_from_the_conv_epilogue, _bn_statistics_of_each_half_of_a_twin_batch, _dev, _rand,
                            _rel)
from test_hip_ops import _conv_bn_fwd_bwd

pytestmark = pytest.mark.gpu
TAPS = (1, 3, 7, 9)
TILE_64, H3_TILE_256 = 1, 6                 # codes of ttts_gemm_tile_choice (include/ttts_hip.h)
# the smallest row count for which ttts_conv1d_fwd_h3_bn_chunk_rows answers 224 at cin = cout = 256 is 32 769 = 99 x 331 (searched
# downwards from the 5-tap case's 48 x 870; the answer depends on the row count alone from three k-tiles on); the smallest with an
# even number of utterances, for a twin batch, is 32 770 = 58 x 565
WIDE_224 = (99, 331, 256, 256)
WIDE_224_TWIN = (58, 565, 256, 256)


def _report(line):
    print(line)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/conv_taps_margin.txt", "a") as f:
        f.write(line + "\n")


def _pad32(c):
    return (c + 31) // 32 * 32


def _conv_wgrad_ref(x, dy, taps):
    """dw (cout, cin, taps) and dbias of a same-padded conv1d by torch's autograd in fp64 (x: (B, T, cin), dy: (B, T, cout))"""
    cout, cin = dy.shape[2], x.shape[2]
    wd = torch.zeros(cout, cin, taps, dtype=torch.float64, device=x.device, requires_grad=True)
    bd = torch.zeros(cout, dtype=torch.float64, device=x.device, requires_grad=True)
    torch.nn.functional.conv1d(x.double().transpose(1, 2), wd, bd, padding=taps // 2).transpose(1, 2).backward(dy.double())
    return wd.grad, bd.grad


def _conv_fwd_ref(x, w, b, taps):
    return torch.nn.functional.conv1d(x.double().transpose(1, 2), w.double(), None if b is None else b.double(),
                                      padding=taps // 2).transpose(1, 2)


def _conv_dgrad_ref(dy, w, taps):
    B, T, _ = dy.shape
    xd = torch.zeros(B, T, w.shape[1], dtype=torch.float64, device=dy.device, requires_grad=True)
    _conv_fwd_ref(xd, w, None, taps).backward(dy.double())
    return xd.grad


# ------------------------------------------------------------------------------------------- a. weight gradient, launches of their own
# (B, T, cin, cout) -> the class ttts_wgrad_group_ok answers at every tap count (the tile of the problem's own fp16x3 plan): 1 the
# 128 x 128 tile, 3 / 4 the 96-wide tiles of 80 input / output channels, 0 no split-precision shape -- all three entries then run
# the fp32-MFMA kernel, on its 64-tile
_SMALL_WGRAD = {(7, 33, 128, 128): 1, (7, 33, 128, 256): 1, (7, 33, 80, 256): 3, (7, 33, 256, 80): 4, (7, 33, 64, 64): 0,
                (7, 33, 64, 20): 0,
                (5, 1, 128, 128): 1}            # T = 1: every tap but the centre is clipped
_WGRAD_CASES = [(*shape, taps, cls) for shape, cls in _SMALL_WGRAD.items() for taps in TAPS] + \
               [(4, 3, 128, 128, 9, 1)]         # T = 3 under a padding of 4: taps that see no row at all


def _wgrad_forms(lib, ops, B, T, cin, cout, taps, forms, label):
    from transformertts_amd.ops import _p, _stream
    M = B * T
    x, dy = _rand(B, T, cin, seed=1), _rand(B, T, cout, seed=2) * 2e-7
    dw_ref, db_ref = _conv_wgrad_ref(x, dy, taps)
    am, xm = ops._amax(dy), ops._amax(x)
    # a destination that is not zero, of the gradient's own magnitude (a larger one would hide the sum's low bits)
    dw0 = _rand(cout, cin, taps, seed=3) * float(dw_ref.abs().max())
    db0 = _rand(cout, seed=4) * float(db_ref.abs().max())
    for form in forms:
        f = getattr(lib, "ttts_conv1d_bwd_weight" + form)
        maxima = (_p(am), _p(xm)) if form == "_h3" else ()
        ws = torch.empty(lib.ttts_wgrad_workspace_bytes(M, cout, cin, taps) // 4, device=_dev())
        dw, db = torch.full((cout, cin, taps), float("nan"), device=_dev()), torch.full((cout,), float("nan"), device=_dev())
        assert f(_p(dy), _p(x), _p(dw), _p(db), _p(ws), ws.numel() * 4, B, T, cin, cout, taps, 0, *maxima, None, _stream()) == 0
        e_w, e_b = _rel(dw, dw_ref), _rel(db, db_ref)
        dw, db = dw0.clone(), db0.clone()
        assert f(_p(dy), _p(x), _p(dw), _p(db), _p(ws), ws.numel() * 4, B, T, cin, cout, taps, 1, *maxima, None, _stream()) == 0
        a_w, a_b = _rel(dw, dw0.double() + dw_ref), _rel(db, db0.double() + db_ref)
        _report(f"wgrad{form or '_f32'} {label}: dw {e_w:.3e} dbias {e_b:.3e} accumulated dw {a_w:.3e} dbias {a_b:.3e}")
        assert e_w < TOL and e_b < TOL and a_w < TOL and a_b < TOL, (form, e_w, e_b, a_w, a_b)


@pytest.mark.parametrize("B,T,cin,cout,taps,cls", _WGRAD_CASES)
def test_conv_weight_gradient_forms_at_other_tap_counts(B, T, cin, cout, taps, cls):
    """ttts_conv1d_bwd_weight, _x6 and _h3 (tap-to-z mapping, per-tap utterance clipping, the [split][tap][co][ci] -> [co][ci][tap]
    second stage): dw and dbias stored, then accumulated onto a non-zero destination."""
    from transformertts_amd import _lib, ops
    lib = _lib.load()
    assert lib.ttts_wgrad_group_ok(B * T, cout, cin, taps) == cls
    assert ops._wgrad_is_split(cout, cin) == (cls != 0)
    _wgrad_forms(lib, ops, B, T, cin, cout, taps, ("", "_x6", "_h3"), f"({B},{T},{cin},{cout}) taps {taps} class {cls}")


# 256-wide outputs over at least 800 k-tiles of 32 rows, at least three tile-taps: the fp16x3 plan takes its 256 x 256 tile
_TILE_256_WGRAD = [(1600, 16, 256, 256, 3, 2), (1600, 16, 256, 256, 9, 2),      # utterances of exactly one 16-row step
                   (1505, 17, 256, 256, 3, 2), (1505, 17, 256, 256, 9, 2),      # 25 585 rows: utterance ends walk through the steps
                   (32, 800, 256, 256, 3, 2), (32, 800, 256, 256, 9, 2),
                   (1596, 16, 256, 256, 3, 1),      # 25 536 rows, 798 k-tiles: the same output on the 128 x 128 register-turning kernel
                   # 320 output channels: a ragged second tile row, so no group takes it (class 0 of a split-precision shape) and
                   # the launch of its own runs the 8-wave register-turning kernel on the 256 x 256 tile
                   (1600, 16, 256, 320, 3, 0), (1600, 16, 256, 320, 9, 0),
                   # utterances of 8 rows: class 2 by its sizes, but the LDS-DMA kernel clips utterances of at least 16 rows only --
                   # the group refuses the member, the launch of its own runs the 8-wave register-turning kernel
                   (3200, 8, 256, 256, 3, 2), (3200, 8, 256, 256, 9, 2)]


@pytest.mark.parametrize("B,T,cin,cout,taps,cls", _TILE_256_WGRAD)
def test_conv_weight_gradient_on_the_256_tile_at_other_tap_counts(B, T, cin, cout, taps, cls):
    """ttts_conv1d_bwd_weight_h3 where the plan takes the 256 x 256 tile: whole tiles by LDS-DMA (wgrad_dma_body: `keep` per row of
    a step, utterance ends anywhere in it), ragged tiles and short utterances on wgrad_h3_kernel<256, 256>."""
    from transformertts_amd import _lib, ops
    lib = _lib.load()
    M = B * T
    assert lib.ttts_wgrad_group_ok(M, cout, cin, taps) == cls and ops._wgrad_is_split(cout, cin)
    assert (-(-M // 32) >= 800) == (cls != 1)
    if T < 16:              # (pointers that are never read: the refusal precedes any launch)
        one = lambda ctype, v: (ctype * 1)(v)       # noqa: E731
        buf = torch.empty(64, device=_dev())
        P = lambda: one(ctypes.c_void_p, buf.data_ptr())        # noqa: E731
        rc = lib.ttts_wgrad_group(1, P(), P(), P(), P(), P(), one(ctypes.c_size_t, 1 << 40), one(ctypes.c_int64, M), one(ctypes.c_int, cout),
                                  one(ctypes.c_int, cin), one(ctypes.c_int, taps), one(ctypes.c_int, T), one(ctypes.c_int, 0), 1, P(), P(),
                                  None, None)
        assert rc == -1 and "needs its utterance length" in _lib.last_error()
    _wgrad_forms(lib, ops, B, T, cin, cout, taps, ("_h3",), f"({B},{T},{cin},{cout}) taps {taps} class {cls}")


# ------------------------------------------------------------------------------------------------------ b. weight gradient, grouped
# member: (cout, cin, taps, kind) -- "conv": taps_i = taps, T_i = T; "conv1": a ONE-tap convolution handed over as the group takes it,
# taps_i = 1 and T_i = 0 (a linear weight; the reference is still conv1d with one tap); "linear": dw = dy^T x
_GROUPS = [
    (1, 7, 33, [(256, 128, 3, "conv"), (128, 256, 9, "conv"), (128, 128, 1, "conv1"), (256, 256, 1, "linear")]),
    (2, 32, 800, [(256, 256, 3, "conv"), (256, 256, 7, "conv")]),
    (3, 7, 33, [(256, 80, 3, "conv"), (256, 80, 9, "conv")]),
    (3, 16, 870, [(256, 80, 3, "conv"), (256, 80, 9, "conv")]),
    (4, 7, 33, [(80, 256, 3, "conv"), (80, 256, 9, "conv")]),
    (4, 16, 870, [(80, 256, 3, "conv"), (80, 256, 9, "conv")]),
]


@pytest.mark.parametrize("cls,B,T,members", _GROUPS, ids=[f"class{g[0]}-{g[1]}-{g[2]}" for g in _GROUPS])
def test_grouped_conv_weight_gradients_of_mixed_tap_counts(cls, B, T, members):
    """ttts_wgrad_group with members of DIFFERENT tap counts in one grid (each member's z range is its own row splits x its own
    taps), every member against fp64; then the same launch with its second stage deferred into a ReduceQueue and flushed (the
    `taps` of the queued convolution reductions): the same bits."""
    from transformertts_amd import _lib, ops
    from transformertts_amd.ops import _stream
    lib, dev = _lib.load(), _dev()
    M, n = B * T, len(members)
    for cout, cin, taps, kind in members:
        assert lib.ttts_wgrad_group_ok(M, cout, cin, taps) == cls, (cout, cin, taps)
    xs = [_rand(B, T, cin, seed=30 + i) for i, (cout, cin, taps, kind) in enumerate(members)]
    dys = [_rand(B, T, cout, seed=40 + i) * (2e-7 if i == 0 else 1.0) for i, (cout, cin, taps, kind) in enumerate(members)]
    refs = []
    for (cout, cin, taps, kind), x, dy in zip(members, xs, dys):
        if kind == "linear":
            refs.append((dy.double().view(M, cout).t() @ x.double().view(M, cin), dy.double().view(M, cout).sum(0)))
        else:
            refs.append(_conv_wgrad_ref(x, dy, taps))
    wss = [torch.empty(lib.ttts_wgrad_workspace_bytes(M, cout, cin, taps) // 4, device=dev) for cout, cin, taps, kind in members]
    ams, xms = [ops._amax(t) for t in dys], [ops._amax(t) for t in xs]
    PA, ZA, LA, IA = ctypes.c_void_p * n, ctypes.c_size_t * n, ctypes.c_int64 * n, ctypes.c_int * n
    ptr = lambda ts: PA(*[t.data_ptr() for t in ts])      # noqa: E731

    def run(queue):
        dws = [torch.zeros(r[0].shape, device=dev) for r in refs]
        dbs = [torch.zeros(m[0], device=dev) for m in members]
        rc = lib.ttts_wgrad_group(n, ptr(dys), ptr(xs), ptr(dws), ptr(dbs), ptr(wss), ZA(*[w.numel() * 4 for w in wss]), LA(*[M] * n),
                                  IA(*[m[0] for m in members]), IA(*[m[1] for m in members]), IA(*[m[2] for m in members]),
                                  IA(*[T if m[3] == "conv" else 0 for m in members]), IA(*[0] * n), 1, ptr(ams), ptr(xms), queue,
                                  _stream())
        assert rc == 0, _lib.last_error()
        return dws, dbs
    dws, dbs = run(None)
    for i, (cout, cin, taps, kind) in enumerate(members):
        e_w, e_b = _rel(dws[i], refs[i][0]), _rel(dbs[i], refs[i][1])
        _report(f"wgrad group class {cls} ({B},{T}) member {i} {cout}x{cin} taps {taps} {kind}: dw {e_w:.3e} dbias {e_b:.3e}")
        assert e_w < TOL and e_b < TOL, (i, e_w, e_b)
    q = ops.ReduceQueue()           # (q.arg() registers an engine callback and is for backward nodes: the handle itself here)
    dws2, dbs2 = run(q.handle)
    assert q.pending() >= n         # nothing reduced yet: the sinks are as they were
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in dws2 + dbs2)
    q.flush()
    assert q.pending() == 0
    assert all(torch.equal(a, b) for a, b in zip(dws + dbs, dws2 + dbs2))


# ------------------------------------------------------------------------------- c. forward and data gradient through the weight image
_FWD_SHAPES = [(3, 50, 128, 256), (2, 7, 256, 128), (5, 1, 128, 128), (4, 33, 80, 64), (2, 9, 20, 64)]


def _fwd_h3(lib, ops, x, w, b, taps, y):
    from transformertts_amd.ops import _p, _stream
    B, T, cin = x.shape
    cout = w.shape[0]
    pl = ops._planes(w, 6, cout, taps * cin, cin, taps)
    return lib.ttts_conv1d_fwd_h3(_p(x), _p(pl), _p(b), _p(y), B, T, cin, cout, taps, _p(ops._amax(x)), None, _stream())


def _dgrad_h3(lib, ops, dy, w, taps, dx):
    from transformertts_amd.ops import _p, _stream
    B, T, cout = dy.shape
    cin = w.shape[1]
    pl = ops._planes(w, 7, cin, taps * cout, cout, taps)
    return lib.ttts_conv1d_bwd_data_h3(_p(dy), _p(pl), _p(dx), B, T, cin, cout, taps, _p(ops._amax(dy)), _stream())


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("B,T,cin,cout", _FWD_SHAPES)
def test_fp16x3_conv_forward_and_data_gradient_at_other_tap_counts(B, T, cin, cout, taps):
    """ttts_conv1d_fwd_h3 and ttts_conv1d_bwd_data_h3 on products computed FROM the weight image (nine taps: two passes of eight;
    80 and 20 channels: every tap padded to 32): the forward at (cin, cout), the data gradient at the shape and at its mirror, so
    that the padded depth is once the input's and once the output's channels; at nine taps the forward again on x * 1e5."""
    from transformertts_amd import _lib, ops
    lib = _lib.load()
    M = B * T
    # (the dispatch sees the image's depth: every tap's channels padded to a multiple of 32)
    assert lib.ttts_gemm_tile_choice(M, cout, taps * _pad32(cin), 2) == TILE_64
    x, w, b = _rand(B, T, cin, seed=1), _rand(cout, cin, taps, seed=2, scale=(taps * cin) ** -0.5), _rand(cout, seed=3)
    y = torch.full((B, T, cout), float("nan"), device=_dev())
    assert _fwd_h3(lib, ops, x, w, b, taps, y) == 0
    e_y = _rel(y, _conv_fwd_ref(x, w, b, taps))
    line = f"conv fwd/dgrad h3 ({B},{T},{cin},{cout}) taps {taps}: y {e_y:.3e}"
    assert e_y < TOL, e_y
    if taps == 9:
        x2 = x * 1e5                                                # any magnitude
        assert _fwd_h3(lib, ops, x2, w, b, taps, y) == 0
        e_big = _rel(y, _conv_fwd_ref(x2, w, b, taps))
        line += f" y(x * 1e5) {e_big:.3e}"
        assert torch.isfinite(y).all() and e_big < TOL, e_big
    for ci, co in ((cin, cout), (cout, cin))[:1 if cin == cout else 2]:
        assert lib.ttts_gemm_tile_choice(M, ci, taps * _pad32(co), 2) == TILE_64
        wg = _rand(co, ci, taps, seed=2, scale=(taps * ci) ** -0.5)
        dy = _rand(B, T, co, seed=3) * 2e-7
        dx = torch.full((B, T, ci), float("nan"), device=_dev())
        assert _dgrad_h3(lib, ops, dy, wg, taps, dx) == 0
        e_dx = _rel(dx, _conv_dgrad_ref(dy, wg, taps))
        line += f" dx(cin {ci}, cout {co}) {e_dx:.3e}"
        assert e_dx < TOL, (ci, co, e_dx)
    _report(line)


@pytest.mark.parametrize("taps", TAPS)
def test_bf16x6_conv_forward_and_data_gradient_at_other_tap_counts(taps):
    """the _x6 forms (three bf16 planes, modes 2 / 3 of ttts_weight_split) at one small shape"""
    from transformertts_amd import _lib, ops
    from transformertts_amd.ops import _p, _stream
    lib = _lib.load()
    B, T, cin, cout = 3, 50, 128, 256
    x, w, b = _rand(B, T, cin, seed=1), _rand(cout, cin, taps, seed=2, scale=(taps * cin) ** -0.5), _rand(cout, seed=3)
    y = torch.full((B, T, cout), float("nan"), device=_dev())
    assert lib.ttts_conv1d_fwd_x6(_p(x), _p(ops._planes(w, 2, cout, taps * cin, cin, taps)), _p(b), _p(y), B, T, cin, cout, taps,
                                  _stream()) == 0
    dy = _rand(B, T, cout, seed=3) * 2e-7
    dx = torch.full((B, T, cin), float("nan"), device=_dev())
    assert lib.ttts_conv1d_bwd_data_x6(_p(dy), _p(ops._planes(w, 3, cin, taps * cout, cout, taps)), _p(dx), B, T, cin, cout, taps,
                                       _stream()) == 0
    e_y, e_dx = _rel(y, _conv_fwd_ref(x, w, b, taps)), _rel(dx, _conv_dgrad_ref(dy, w, taps))
    _report(f"conv fwd/dgrad x6 ({B},{T},{cin},{cout}) taps {taps}: y {e_y:.3e} dx {e_dx:.3e}")
    assert e_y < TOL and e_dx < TOL, (e_y, e_dx)


@pytest.mark.parametrize("taps", [3, 9])
def test_fp16x3_conv_on_the_224_row_tile_at_other_tap_counts(taps):
    """the one-wave-per-SIMD 256 x 256 tile with the clipping loader (224 rows a tile) at the smallest row count that takes it:
    utterances of 331 rows end inside the tiles; forward and data gradient (cin = cout: one shape)."""
    from transformertts_amd import _lib, ops
    lib = _lib.load()
    B, T, cin, cout = WIDE_224
    assert lib.ttts_gemm_tile_choice(B * T, cout, taps * cin, 2) == H3_TILE_256
    assert lib.ttts_conv1d_fwd_h3_bn_chunk_rows(B, T, cin, cout, taps) == 224
    assert lib.ttts_conv1d_fwd_h3_bn_chunk_rows(1, B * T - 1, cin, cout, taps) != 224       # (one row fewer: another tile)
    x, w, b = _rand(B, T, cin, seed=1), _rand(cout, cin, taps, seed=2, scale=(taps * cin) ** -0.5), _rand(cout, seed=3)
    y = torch.full((B, T, cout), float("nan"), device=_dev())
    assert _fwd_h3(lib, ops, x, w, b, taps, y) == 0
    e_y = _rel(y, _conv_fwd_ref(x, w, b, taps))
    del x
    dy = _rand(B, T, cout, seed=3) * 2e-7
    dx = torch.full((B, T, cin), float("nan"), device=_dev())
    assert _dgrad_h3(lib, ops, dy, w, taps, dx) == 0
    e_dx = _rel(dx, _conv_dgrad_ref(dy, w, taps))
    _report(f"conv fwd/dgrad h3 224-row tile ({B},{T},{cin},{cout}) taps {taps}: y {e_y:.3e} dx {e_dx:.3e}")
    assert e_y < TOL and e_dx < TOL, (e_y, e_dx)


# The forward / data-gradient tile follows the rows and the width; the two-workgroup 256 x 128 tile is a candidate up to a depth of
# 512 only, so at 128 channels one and three taps take it where seven and nine take the 256 x 256 tile (its 224-row variant).
# (B, T, cin, cout, taps, forward tile, data-gradient tile): 3 = 64 x 128, 4 = 128 x 96, 6 = 256 x 256, 7 = 256 x 128 (8 waves),
# 8 = 256 x 128 (4 waves, two workgroups per CU)
_LARGER_TILES = [(99, 331, 128, 256, 1, 8, 7), (99, 331, 128, 256, 3, 8, 7), (99, 331, 128, 256, 7, 6, 7), (99, 331, 128, 256, 9, 6, 7),
                 (6, 833, 64, 512, 3, 3, 1), (6, 833, 64, 512, 9, 3, 1), (11, 833, 64, 512, 3, 7, 1), (11, 833, 64, 512, 9, 7, 1),
                 (57, 870, 64, 80, 3, 4, 4), (57, 870, 64, 80, 9, 4, 4)]


@pytest.mark.parametrize("B,T,cin,cout,taps,fwd_tile,bwd_tile", _LARGER_TILES)
def test_fp16x3_conv_on_the_larger_tiles_at_other_tap_counts(B, T, cin, cout, taps, fwd_tile, bwd_tile):
    """every other tile of the forward-type dispatch at the smallest row counts that reach it: forward and data gradient"""
    from transformertts_amd import _lib, ops
    lib = _lib.load()
    M = B * T
    assert lib.ttts_gemm_tile_choice(M, cout, taps * _pad32(cin), 2) == fwd_tile
    assert lib.ttts_gemm_tile_choice(M, cin, taps * _pad32(cout), 2) == bwd_tile
    x, w, b = _rand(B, T, cin, seed=1), _rand(cout, cin, taps, seed=2, scale=(taps * cin) ** -0.5), _rand(cout, seed=3)
    y = torch.full((B, T, cout), float("nan"), device=_dev())
    assert _fwd_h3(lib, ops, x, w, b, taps, y) == 0
    e_y = _rel(y, _conv_fwd_ref(x, w, b, taps))
    del x
    dy = _rand(B, T, cout, seed=3) * 2e-7
    dx = torch.full((B, T, cin), float("nan"), device=_dev())
    assert _dgrad_h3(lib, ops, dy, w, taps, dx) == 0
    e_dx = _rel(dx, _conv_dgrad_ref(dy, w, taps))
    _report(f"conv fwd/dgrad h3 tiles {fwd_tile}/{bwd_tile} ({B},{T},{cin},{cout}) taps {taps}: y {e_y:.3e} dx {e_dx:.3e}")
    assert e_y < TOL and e_dx < TOL, (e_y, e_dx)


# ---------------------------------------------------------------------------------------- d. BatchNorm statistics from the epilogue
# (B, T, cin, cout, offset, taps, rows a partial covers, partials): 32-row chunks of the 64 x 64 tile (two a tile), the 224-row tile
# (one), and at 128 channels the 128-row chunks of the two-workgroup 256 x 128 tile at three taps against the 224-row tile at nine
_BN_EPILOGUE = [c for taps in (3, 9) for c in [(3, 50, 128, 256, 0.0, taps, 32, 6), (2, 7, 256, 128, 40.0, taps, 32, 2),
                                               (*WIDE_224, 3.0, taps, 224, 147)]] + \
               [(99, 331, 128, 256, 0.0, 3, 128, 258), (99, 331, 128, 256, 0.0, 9, 224, 147)]


@pytest.mark.parametrize("B,T,cin,cout,offset,taps,chunk,nblk", _BN_EPILOGUE)
def test_batchnorm_statistics_from_the_conv_epilogue_at_other_tap_counts(B, T, cin, cout, offset, taps, chunk, nblk):
    """the body of test_batchnorm_statistics_from_the_conv_epilogue (tests/test_hip_modes.py) at 3 and 9 taps"""
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_conv1d_fwd_h3_bn_chunk_rows(B, T, cin, cout, taps) == chunk
    assert lib.ttts_conv1d_fwd_h3_bn_blocks(B, T, cin, cout, taps) == nblk
    label = f"bn epilogue ({B},{T},{cin},{cout}) offset {offset:g} taps {taps}"
    _bn_statistics_from_the_conv_epilogue(B, T, cin, cout, offset, taps, report=lambda s: _report(f"{label}: {s}"))


@pytest.mark.parametrize("taps", [3, 9])
@pytest.mark.parametrize("B,T,cin,cout,offset,chunk", [(6, 50, 128, 256, 0.0, 32), (4, 7, 256, 128, 40.0, 32),
                                                       (*WIDE_224_TWIN, 3.0, 224)])
def test_batchnorm_statistics_of_each_half_of_a_twin_batch_at_other_tap_counts(B, T, cin, cout, offset, chunk, taps):
    """the body of test_batchnorm_statistics_of_each_half_of_a_twin_batch at 3 and 9 taps; in each shape the halves share a chunk"""
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_conv1d_fwd_h3_bn_chunk_rows(B, T, cin, cout, taps) == chunk and (B * T // 2) % chunk != 0
    label = f"bn twin ({B},{T},{cin},{cout}) offset {offset:g} taps {taps}"
    _bn_statistics_of_each_half_of_a_twin_batch(B, T, cin, cout, offset, taps, report=lambda s: _report(f"{label}: {s}"))


# ---------------------------------------------------------------------------------------------------------- e. ops.conv_bn end to end
# (B, T, cin, cout, act) -> (BatchNorm partials of the forward, class of the weight gradient; 0: the fp32-MFMA kernel behind _x6)
_CONV_BN = {(3, 37, 128, 128, 0): (4, 1), (2, 131, 256, 80, 0): (10, 4), (2, 64, 80, 256, 2): (4, 3), (5, 1, 16, 128, 2): (2, 0)}


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("B,T,cin,cout,act", list(_CONV_BN))
def test_conv_bn_fwd_bwd_at_other_tap_counts(B, T, cin, cout, act, taps):
    """the body of test_conv_bn_fwd_bwd (tests/test_hip_ops.py): convolution with the epilogue's partials -> statistics ->
    normalisation (+ tanh), and backward BatchNorm -> data gradient -> weight gradient"""
    from transformertts_amd import _lib, ops
    lib = _lib.load()
    nblk, cls = _CONV_BN[(B, T, cin, cout, act)]
    assert ops._h3_shape_ok(taps * cin, cout, cin) and ops._h3_shape_ok(taps * cout, cin, cout)
    assert lib.ttts_gemm_tile_choice(B * T, cout, taps * _pad32(cin), 2) == TILE_64
    assert lib.ttts_gemm_tile_choice(B * T, cin, taps * _pad32(cout), 2) == TILE_64
    assert lib.ttts_conv1d_fwd_h3_bn_blocks(B, T, cin, cout, taps) == nblk
    assert lib.ttts_conv1d_fwd_h3_bn_chunk_rows(B, T, cin, cout, taps) == 32
    assert lib.ttts_wgrad_group_ok(B * T, cout, cin, taps) == cls and ops._wgrad_is_split(cout, cin) == (cls != 0)
    label = f"conv_bn ({B},{T},{cin},{cout}) act {act} taps {taps}"
    _conv_bn_fwd_bwd(B, T, cin, cout, act, True, taps, report=lambda s: _report(f"{label}: {s}"))
