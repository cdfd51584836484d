"""Every refresh path of the weight-image cache (transformertts_amd/ops.py: the lazy process-wide refresh, `PlaneTable.refresh`,
a stack's own table, the single re-split) writes the image a first split of the same numbers writes -- bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"lin": (96, 64), "conv": (32, 32, 5), "kv": (192, 64)}      # the smallest the modes take: depths and stacked rows % 32 == 0
SCALES = {"lin": 1.0, "conv": 0.02, "kv": 30.0}                       # (neighbours in a table whose maxima differ)


def _model():
    sizes = {k: int(torch.Size(s).numel()) for k, s in SHAPES.items()}
    flat = torch.zeros(sum(sizes.values()), device="cuda")
    mod, off = torch.nn.Module(), 0
    for k, shape in SHAPES.items():
        p = torch.nn.Parameter(torch.empty(0, device="cuda"))
        p.data = flat[off:off + sizes[k]].view(shape)                 # as optim.FlatAdam lays parameters out
        mod.register_parameter(k, p)
        off += sizes[k]
    return mod


def _images(ops, lin, conv, kv, owner):
    """every image of the three weights, as the ops ask for them: {name: tensor}"""
    out = {}
    for mode in (ops.H3_LIN_FWD, ops.H3D_LIN_FWD):
        out["lin", mode] = ops._planes(lin, mode, 96, 64)
    for mode in (ops.H3_LIN_BWD, ops.H3D_LIN_BWD):
        out["lin", mode] = ops._planes(lin, mode, 64, 96)
    for mode in (ops.H3_CONV_FWD, ops.H3_CONV_BWD):
        out["conv", mode] = ops._planes(conv, mode, 32, 160, 32, 5)
    slices = [ops.param_rows(kv, 0, 64), ops.param_rows(kv, 64, 128)]
    for i, sl in enumerate(slices):
        out["kv", i, ops.H3_LIN_FWD] = ops._planes(sl, ops.H3_LIN_FWD, 64, 64)
    for mode in (ops.H3D_LIN_FWD, ops.H3_LIN_BWD):
        out["stack", mode] = ops._stacked_planes(owner, slices, mode)
    return out


def _fresh(ops, mod):
    """the same images over clones of the weights: clones carry no cache, so every one of them is a first split"""
    return {k: v.clone() for k, v in _images(ops, mod.lin.detach().clone(), mod.conv.detach().clone(), mod.kv.detach().clone(),
                                             torch.nn.Module()).items()}


def _new_values(ops, mod, gen):
    for k, p in mod.named_parameters():
        p.data.copy_(torch.randn(p.shape, device="cuda", generator=gen) * SCALES[k])     # (no version counter sees this)
    mod.kv.data[64:128] *= 0.01                      # the second slice alone scales otherwise than the stack it is a window of
    ops.bump_param_epoch()


def _assert_same(got, want, what):
    """every word a split writes: the two planes and max|w|, the first float of the 16-byte tail (ttts_split_image_bytes); nothing
    writes the tail's other 12 bytes, which are whatever the allocator handed out"""
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].numel() == want[k].numel() and torch.equal(got[k][:-6], want[k][:-6]), (what, k)


def test_every_refresh_path_writes_the_image_a_fresh_split_writes(monkeypatch):
    from transformertts_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    mod = _model()
    use = lambda: _images(ops, mod.lin, mod.conv, mod.kv, mod)
    _new_values(ops, mod, gen)
    first = use()
    _assert_same(first, _fresh(ops, mod), "first use")
    _new_values(ops, mod, gen)                       # the lazy path: the first use refreshes the model with one launch
    lazy = use()
    assert all(lazy[k] is first[k] for k in first)
    _assert_same(lazy, _fresh(ops, mod), "process-wide refresh")
    _new_values(ops, mod, gen)
    ops.PlaneTable(mod).refresh()
    _assert_same(use(), _fresh(ops, mod), "PlaneTable.refresh")
    _new_values(ops, mod, gen)                       # no batching: each stack by its own table, every other image by a single split
    monkeypatch.setattr(ops, "_BATCHED_SPLIT", False)
    _assert_same(use(), _fresh(ops, mod), "single splits and the stacks' own tables")
    torch.cuda.synchronize()
