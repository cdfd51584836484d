"""The bookkeeping of the split-precision weight images ("planes", transformertts_amd/ops.py): which `ttts_weight_split` and
`ttts_weight_split_batched` calls `ops._planes`, `ops.PlaneTable` and `ops._stacked_planes` make, and with which descriptor rows,
recorded on the CPU against a stand-in library.  Host logic only, no GPU: parameters are CPU views of one flat tensor per model,
as `optim.FlatAdam` lays them out.

A record is ("split", source, image, rows, cols, mode, c2, taps) or ("batched", entries, work units, rows), a row being
[source, image, rows, cols, mode, c2, taps, first work unit] as the kernel reads it.  Addresses are written symbolically: a source
is (model, element offset in its flat tensor), an image is its number in order of first appearance.  The stand-in sizes an image
at rows * cols 16-bit words and counts (rows + 31) // 32 + c2 work units for an entry, so a packed window geometry that leaked
into the count would show."""
import gc

import pytest

LIN, CONV, KV = (96, 64), (32, 32, 5), (192, 64)
CAPTURE_WORDING = "weight planes must exist before a HIP-graph capture: run the eager warm-up steps first"


def _pack(hi, lo):
    return (hi << 32) | lo


class _Recorder:
    def __init__(self, torch):
        self.torch, self.log, self.capturing, self.flats, self.images, self.keep = torch, [], False, {}, {}, []

    def model(self, name, **shapes):
        """a module whose parameters are views of one flat tensor, in the order given"""
        torch = self.torch
        sizes = {k: int(torch.Size(s).numel()) for k, s in shapes.items()}
        flat = torch.arange(sum(sizes.values()), dtype=torch.float32)
        self.flats[name] = flat
        mod, off = torch.nn.Module(), 0
        for k, shape in shapes.items():
            p = torch.nn.Parameter(torch.empty(0))
            p.data = flat[off:off + sizes[k]].view(shape)
            mod.register_parameter(k, p)
            off += sizes[k]
        return mod

    def source(self, addr):
        for name, flat in self.flats.items():
            if flat.data_ptr() <= addr < flat.data_ptr() + 4 * flat.numel():
                return (name, (addr - flat.data_ptr()) // 4)
        return ("?", addr)

    def image(self, addr):
        return self.images.setdefault(addr, len(self.images))

    def take(self):
        log, self.log = self.log, []
        return log

    def install(self, mp, ops, _lib):
        rec, torch = self, self.torch

        class Lib:
            @staticmethod
            def ttts_split_image_bytes(rows, cols, mode, c2, taps):
                return 2 * rows * cols

            @staticmethod
            def ttts_weight_split_units(rows, cols, mode, c2):
                return (rows + 31) // 32 + c2

            @staticmethod
            def ttts_weight_split(w, planes, rows, cols, mode, c2, taps, stream):
                rec.keep.append(planes)           # (an image the cache dropped keeps its address to itself)
                rec.log.append(("split", rec.source(w.data_ptr()), rec.image(planes.data_ptr()), rows, cols, mode, c2, taps))
                return 0

            @staticmethod
            def ttts_weight_split_batched(table, n, units, stream):
                rows = [[rec.source(r[0]), rec.image(r[1])] + r[2:] for r in table.tolist()]
                rec.log.append(("batched", n, units, rows))
                return 0

        lib = Lib()
        mp.setattr(_lib, "load", lambda: lib)
        mp.setattr(ops, "_stream", lambda: None)
        mp.setattr(ops, "_p", lambda t: t)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: rec.capturing)
        mp.setattr(torch.Tensor, "pin_memory", lambda t: t)
        mp.setattr(ops, "_plane_entries", [])


@pytest.fixture
def env(monkeypatch):
    import torch
    from transformertts_amd import _lib, ops
    rec = _Recorder(torch)
    rec.install(monkeypatch, ops, _lib)
    return rec, ops, torch


def _lin(ops, w, mode):
    n, k = w.shape
    return ops._planes(w, mode, n, k) if mode in (ops.H3_LIN_FWD, ops.H3D_LIN_FWD) else ops._planes(w, mode, k, n)


def _conv(ops, w, mode):
    cout, cin, taps = w.shape
    if mode == ops.H3_CONV_FWD:
        return ops._planes(w, mode, cout, taps * cin, cin, taps)
    return ops._planes(w, mode, cin, taps * cout, cout, taps)


def test_first_use_splits_each_weight_and_mode_once(env):
    rec, ops, torch = env
    A = rec.model("A", lin=LIN, conv=CONV)
    first = [_lin(ops, A.lin, ops.H3_LIN_FWD), _lin(ops, A.lin, ops.H3_LIN_BWD), _conv(ops, A.conv, ops.H3_CONV_FWD)]
    assert rec.take() == [("split", ("A", 0), 0, 96, 64, 4, 0, 0),
                          ("split", ("A", 0), 1, 64, 96, 5, 0, 0),
                          ("split", ("A", 6144), 2, 32, 160, 6, 32, 5)]
    assert [p.numel() for p in first] == [96 * 64, 64 * 96, 32 * 160] and all(p.dtype == torch.int16 for p in first)
    again = [_lin(ops, A.lin, ops.H3_LIN_FWD), _lin(ops, A.lin, ops.H3_LIN_BWD), _conv(ops, A.conv, ops.H3_CONV_FWD)]
    assert rec.take() == []
    assert all(a is b for a, b in zip(first, again))
    assert sorted(A.lin._ttts_planes) == [(4, 0), (5, 0)] and sorted(A.conv._ttts_planes) == [(6, 0)]


def test_an_epoch_bump_refreshes_one_model_with_one_launch(env):
    rec, ops, torch = env
    A, B = rec.model("A", lin=LIN, conv=CONV), rec.model("B", lin=LIN, conv=CONV)
    _lin(ops, A.lin, 4), _lin(ops, B.lin, 4), _lin(ops, A.lin, 5), _conv(ops, B.conv, 7), _conv(ops, A.conv, 6)
    assert [r[:3] for r in rec.take()] == [("split", ("A", 0), 0), ("split", ("B", 0), 1), ("split", ("A", 0), 2),
                                           ("split", ("B", 6144), 3), ("split", ("A", 6144), 4)]
    ops.bump_param_epoch()
    _conv(ops, A.conv, 6)
    assert rec.take() == [("batched", 3, 38, [[("A", 0), 0, 96, 64, 4, 0, 0, 0],
                                              [("A", 0), 2, 64, 96, 5, 0, 0, 3],
                                              [("A", 6144), 4, 32, 160, 6, 32, 5, 5]])]
    _lin(ops, A.lin, 4), _lin(ops, A.lin, 5), _conv(ops, A.conv, 6)
    assert rec.take() == []
    _lin(ops, B.lin, 4)
    assert rec.take() == [("batched", 2, 36, [[("B", 0), 1, 96, 64, 4, 0, 0, 0],
                                              [("B", 6144), 3, 32, 160, 7, 32, 5, 3]])]
    _conv(ops, B.conv, 7), _lin(ops, A.lin, 4)
    assert rec.take() == []
    ops.bump_param_epoch()                      # the same entries again: the same rows
    _lin(ops, A.lin, 5)
    assert rec.take() == [("batched", 3, 38, [[("A", 0), 0, 96, 64, 4, 0, 0, 0],
                                              [("A", 0), 2, 64, 96, 5, 0, 0, 3],
                                              [("A", 6144), 4, 32, 160, 6, 32, 5, 5]])]


def test_a_moved_version_or_address_is_a_single_split_never_a_batched_one(env):
    rec, ops, torch = env
    A = rec.model("A", lin=LIN, conv=CONV)
    img = _lin(ops, A.lin, 4)
    _conv(ops, A.conv, 6)
    rec.take()
    with torch.no_grad():
        A.lin.add_(1.0)
    assert _lin(ops, A.lin, 4) is img           # the same buffer, written again
    _conv(ops, A.conv, 6)
    assert rec.take() == [("split", ("A", 0), 0, 96, 64, 4, 0, 0)]
    rec.flats["A2"] = torch.zeros(LIN)
    A.lin.data = rec.flats["A2"]
    assert _lin(ops, A.lin, 4) is img
    assert rec.take() == [("split", ("A2", 0), 0, 96, 64, 4, 0, 0)]
    _lin(ops, A.lin, 4)
    assert rec.take() == []
    # the epoch AND the version moved: the batched refresh leaves that weight out, its own use re-splits it
    A.conv.data = rec.flats["A2"].new_zeros(CONV)
    rec.flats["A3"] = A.conv.data
    _conv(ops, A.conv, 6)
    assert rec.take() == [("split", ("A3", 0), 1, 32, 160, 6, 32, 5)]
    A.lin.data = rec.flats["A"][:6144].view(LIN)
    _lin(ops, A.lin, 4), _lin(ops, A.lin, 5)
    rec.take()
    A.conv.data = rec.flats["A"][6144:].view(CONV)
    _conv(ops, A.conv, 6)
    rec.take()
    ops.bump_param_epoch()
    with torch.no_grad():
        A.lin.mul_(2.0)
    _conv(ops, A.conv, 6)
    assert rec.take() == [("batched", 1, 33, [[("A", 6144), 1, 32, 160, 6, 32, 5, 0]])]
    _lin(ops, A.lin, 5), _lin(ops, A.lin, 4)
    assert rec.take() == [("split", ("A", 0), 2, 64, 96, 5, 0, 0), ("split", ("A", 0), 0, 96, 64, 4, 0, 0)]
    _lin(ops, A.lin, 5), _lin(ops, A.lin, 4), _conv(ops, A.conv, 6)
    assert rec.take() == []


def test_inside_a_capture_nothing_is_batched_and_nothing_is_allocated(env):
    rec, ops, torch = env
    A = rec.model("A", lin=LIN, conv=CONV)
    img = _lin(ops, A.lin, 4)
    _conv(ops, A.conv, 6)
    rec.take()
    ops.bump_param_epoch()
    rec.capturing = True
    assert _lin(ops, A.lin, 4) is img           # the launch PlaneTable.mark_current exists to avoid
    assert rec.take() == [("split", ("A", 0), 0, 96, 64, 4, 0, 0)]
    with pytest.raises(RuntimeError, match=CAPTURE_WORDING):
        _lin(ops, A.lin, 5)
    assert rec.take() == [] and sorted(A.lin._ttts_planes) == [(4, 0)]
    rec.capturing = False
    _conv(ops, A.conv, 6)
    assert rec.take() == [("batched", 1, 33, [[("A", 6144), 1, 32, 160, 6, 32, 5, 0]])]
    _lin(ops, A.lin, 4)
    assert rec.take() == []


def test_plane_table(env, monkeypatch):
    rec, ops, torch = env
    A = rec.model("A", lin=LIN, conv=CONV)
    with pytest.raises(RuntimeError, match="the module has no weight planes yet"):
        ops.PlaneTable(A)
    _lin(ops, A.lin, 4), _lin(ops, A.lin, 5), _conv(ops, A.conv, 6)
    rec.take()
    rows = [[("A", 0), 0, 96, 64, 4, 0, 0, 0], [("A", 0), 1, 64, 96, 5, 0, 0, 3], [("A", 6144), 2, 32, 160, 6, 32, 5, 5]]
    use_all = lambda: (_lin(ops, A.lin, 4), _lin(ops, A.lin, 5), _conv(ops, A.conv, 6))
    t = ops.PlaneTable(A)
    assert t.valid() and not t.stale() and rec.take() == []
    ops.bump_param_epoch()
    assert t.valid() and t.stale()
    t.refresh()
    assert rec.take() == [("batched", 3, 38, rows)]
    assert not t.stale()
    use_all()
    assert rec.take() == []
    t.mark_stale()
    assert t.stale() and t.valid()
    _lin(ops, A.lin, 5)                         # eager: the process-wide refresh serves all three
    assert rec.take() == [("batched", 3, 38, rows)]
    assert not t.stale()
    t.mark_stale()
    t.mark_current()
    assert not t.stale()
    use_all()
    assert rec.take() == []
    t.mark_stale()                              # as after a capture; a refresh recorded in the next one covers it
    rec.capturing = True
    t.refresh()
    use_all()
    rec.capturing = False
    assert rec.take() == [("batched", 3, 38, rows)]
    # an image re-allocated behind the table (here: the same weight asked for at another size, single splits only)
    monkeypatch.setattr(ops, "_BATCHED_SPLIT", False)
    ops.bump_param_epoch()
    assert t.valid()
    ops._planes(A.lin, 4, 48, 64)
    assert rec.take() == [("split", ("A", 0), 3, 48, 64, 4, 0, 0)]
    assert not t.valid()
    monkeypatch.setattr(ops, "_BATCHED_SPLIT", True)
    t = ops.PlaneTable(A)
    assert t.valid() and t.stale()
    t.refresh()
    assert rec.take() == [("batched", 3, 37, [[("A", 0), 3, 48, 64, 4, 0, 0, 0], [("A", 0), 1, 64, 96, 5, 0, 0, 2],
                                              [("A", 6144), 2, 32, 160, 6, 32, 5, 4]])]
    with torch.no_grad():
        A.conv.add_(1.0)
    assert not t.valid() and not t.stale()


def test_row_slices_are_cached_on_the_parameter_they_were_cut_from(env):
    rec, ops, torch = env
    A = rec.model("A", kv=KV, lin=LIN)
    s1 = ops.param_rows(A.kv, 64, 128)
    img = ops._planes(s1, 4, 64, 64)
    assert rec.take() == [("split", ("A", 4096), 0, 64, 64, 4, 0, 0)]
    assert sorted(A.kv._ttts_planes) == [(4, 64)] and not hasattr(s1, "_ttts_planes")
    ent = A.kv._ttts_planes[(4, 64)]
    assert ent.planes is img and ent.wref() is A.kv and ent.off == 4096 * 4
    assert ops._planes(ops.param_rows(A.kv, 64, 128), 4, 64, 64) is img and rec.take() == []
    ops._planes(ops.param_rows(A.kv, 0, 64), 4, 64, 64)
    assert rec.take() == [("split", ("A", 0), 1, 64, 64, 4, 0, 0)]
    ops.bump_param_epoch()
    assert ops._planes(ops.param_rows(A.kv, 64, 128), 4, 64, 64) is img
    assert rec.take() == [("batched", 2, 4, [[("A", 4096), 0, 64, 64, 4, 0, 0, 0], [("A", 0), 1, 64, 64, 4, 0, 0, 2]])]
    t = ops.PlaneTable(A)
    ops.bump_param_epoch()
    t.refresh()
    assert rec.take() == [("batched", 2, 4, [[("A", 4096), 0, 64, 64, 4, 0, 0, 0], [("A", 0), 1, 64, 64, 4, 0, 0, 2]])]


def test_stacked_images(env):
    rec, ops, torch = env
    A = rec.model("A", kv=KV, lin=LIN)
    slices = lambda: [ops.param_rows(A.kv, 0, 64), ops.param_rows(A.kv, 64, 128)]
    _lin(ops, A.lin, 4)
    fwd = ops._stacked_planes(A, slices(), ops.H3D_LIN_FWD)
    bwd = ops._stacked_planes(A, slices(), ops.H3_LIN_BWD)
    fwd_rows = [[("A", 0), 1, 64, 64, 8, _pack(128, 64), _pack(0, 0), 0], [("A", 4096), 1, 64, 64, 8, _pack(128, 64), _pack(64, 0), 2]]
    bwd_rows = [[("A", 0), 2, 64, 64, 5, _pack(64, 128), _pack(0, 0), 0], [("A", 4096), 2, 64, 64, 5, _pack(64, 128), _pack(0, 64), 2]]
    assert rec.take() == [("split", ("A", 12288), 0, 96, 64, 4, 0, 0), ("batched", 2, 4, fwd_rows), ("batched", 2, 4, bwd_rows)]
    assert fwd.numel() == bwd.numel() == 128 * 64
    assert ops._stacked_planes(A, slices(), ops.H3D_LIN_FWD) is fwd and ops._stacked_planes(A, slices(), ops.H3_LIN_BWD) is bwd
    assert rec.take() == []
    # the optimizer stepped: one launch for the model, the windows among its other entries
    ops.bump_param_epoch()
    assert ops._stacked_planes(A, slices(), ops.H3_LIN_BWD) is bwd
    both = [[("A", 12288), 0, 96, 64, 4, 0, 0, 0]] + [r[:7] + [3 + r[7]] for r in fwd_rows] + [r[:7] + [7 + r[7]] for r in bwd_rows]
    assert rec.take() == [("batched", 5, 11, both)]
    ops._stacked_planes(A, slices(), ops.H3D_LIN_FWD), _lin(ops, A.lin, 4)
    assert rec.take() == []
    ops.bump_param_epoch()
    _lin(ops, A.lin, 4)
    assert rec.take() == [("batched", 5, 11, both)]
    ops._stacked_planes(A, slices(), ops.H3D_LIN_FWD), ops._stacked_planes(A, slices(), ops.H3_LIN_BWD)
    assert rec.take() == []
    t = ops.PlaneTable(A)
    ops.bump_param_epoch()
    t.refresh()
    kv_first = [r[:7] + [r[7]] for r in fwd_rows] + [r[:7] + [4 + r[7]] for r in bwd_rows] + [[("A", 12288), 0, 96, 64, 4, 0, 0, 8]]
    assert rec.take() == [("batched", 5, 11, kv_first)]
    # inside a capture: an epoch-stale stack is re-split by its own table, a missing one refuses
    ops.bump_param_epoch()
    rec.capturing = True
    assert ops._stacked_planes(A, slices(), ops.H3D_LIN_FWD) is fwd
    assert rec.take() == [("batched", 2, 4, fwd_rows)]
    other = torch.nn.Module()
    with pytest.raises(RuntimeError, match="stacked " + CAPTURE_WORDING):
        ops._stacked_planes(other, slices(), ops.H3D_LIN_FWD)
    rec.capturing = False
    _lin(ops, A.lin, 4)
    assert rec.take() == [("batched", 3, 7, [[("A", 12288), 0, 96, 64, 4, 0, 0, 0]] + [r[:7] + [3 + r[7]] for r in bwd_rows])]
    # slices that moved (cut at other rows): a new stack
    moved = lambda: [ops.param_rows(A.kv, 64, 128), ops.param_rows(A.kv, 128, 192)]
    fwd2 = ops._stacked_planes(A, moved(), ops.H3D_LIN_FWD)
    assert fwd2 is not fwd
    assert rec.take() == [("batched", 2, 4, [[("A", 4096), 3] + fwd_rows[0][2:], [("A", 8192), 3] + fwd_rows[1][2:]])]
    assert ops._stacked_planes(A, moved(), ops.H3D_LIN_FWD) is fwd2 and rec.take() == []
    with pytest.raises(ValueError):
        ops._stacked_planes(other, [ops.param_rows(A.kv, 0, 48), ops.param_rows(A.kv, 48, 96)], ops.H3_LIN_BWD)
    assert rec.take() == []


def test_dead_weights_leave_the_registry(env):
    rec, ops, torch = env
    A, B = rec.model("A", lin=LIN, conv=CONV), rec.model("B", lin=LIN, conv=CONV)
    _lin(ops, A.lin, 4), _lin(ops, B.lin, 4), _conv(ops, B.conv, 6), _conv(ops, A.conv, 6)
    assert len(ops._plane_entries) == 4
    rec.take()
    del B
    gc.collect()
    ops.bump_param_epoch()
    _lin(ops, A.lin, 4)
    assert rec.take() == [("batched", 2, 36, [[("A", 0), 0, 96, 64, 4, 0, 0, 0], [("A", 6144), 3, 32, 160, 6, 32, 5, 3]])]
    assert len(ops._plane_entries) == 2 and all(e.wref() is p for e, p in zip(ops._plane_entries, (A.lin, A.conv)))
