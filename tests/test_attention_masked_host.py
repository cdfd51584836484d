"""The masked 128-column attention entry points (ABI v18, csrc/attention_wide.hip): declared, bound, exported, and their
refusals; and the per-tensor memory of what a mask resolves to (model/layers.py `_MaskMemo`).  Host logic only, no GPU (every
refusal happens before a launch)."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_attention_fwd_wide_masked", "ttts_attention_bwd_wide_masked")
MASK_ARGS = ("add_mask", "ldm", "mask_stride_b", "mask_stride_h", "key_dead", "ldd")


def test_abi_version_and_the_header_declares_the_masked_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 18
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    P, L = ctypes.c_void_p, ctypes.c_int64
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        # the arguments of the _wide entry point, then the six mask arguments, then the stream
        res, args = _lib.SIGNATURES[name]
        res0, args0 = _lib.SIGNATURES[name[:-len("_masked")]]
        assert res == res0 and args == args0[:-1] + [P, L, L, L, P, L] + args0[-1:]
        # ... and the header says so, with the torch call site it replaces
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert [a.split()[-1].lstrip("*") for a in decl.split(",")][-7:-1] == list(MASK_ARGS)
    assert "torch/nn/functional.py" in hdr[hdr.index("ABI v18"):hdr.index("int ttts_attention_fwd_wide_masked")]


def test_masked_entry_points_refuse_bad_arguments_with_a_message():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a4 = ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    dims = dict(B=1, H=2, Tq=5, Tk=5, ldq=768, ldk=768, ldv=768, ldo=256)
    grads = dict(lddq=768, lddk=768, lddv=768)
    tail = dict(causal=0, scale=0.1, p=0.0, seed=0, step_seed=None)
    mask = dict(add_mask=a, ldm=8, mask_stride_b=0, mask_stride_h=0, key_dead=a, ldd=5)
    ptrs = {n: a for n in ("q", "k", "v", "o", "d_o", "stat", "delta", "dq", "dk", "dv", "lens")}
    defaults = dict(ptrs, **dims, **grads, **tail, **mask)
    fwd_order = ["q", "k", "v", "o", "stat", "attn", "lens"] + list(dims) + list(tail) + list(mask) + ["stream"]
    bwd_order = (["q", "k", "v", "o", "d_o", "stat", "delta", "dq", "dk", "dv", "lens"] + list(dims) + list(grads) + list(tail) +
                 list(mask) + ["stream"])

    def caller(fn, order):
        def call(**kw):
            unknown = set(kw) - set(order)
            assert not unknown, unknown
            return getattr(lib, fn)(*[kw.get(name, defaults.get(name)) for name in order])
        return call

    fwd, bwd = caller(NEW[0], fwd_order), caller(NEW[1], bwd_order)
    for call, name in ((fwd, "attention_fwd_wide_masked"), (bwd, "attention_bwd_wide_masked")):
        # the shared check (attn_check), under this entry point's name
        bad(call(q=None), name + ": null pointer")
        bad(call(stat=None), name + ": null pointer")
        bad(call(lens=None), name + ": null pointer")
        bad(call(B=0), name + ": sizes must be positive (B 0,")
        bad(call(ldq=770), "multiples of 4 floats (ldq 770,")
        bad(call(ldk=128), ">= H*128 = 256 (ldq 768, ldk 128,")
        bad(call(p=1.0), "dropout p 1 is outside [0, 1)")
        bad(call(causal=1, Tk=6, ldd=6), "causal form needs Tq == Tk (Tq 5, Tk 6)")
        bad(call(k=a4), "16-byte aligned")
        # the mask operands, each refusal naming the value
        bad(call(add_mask=None, key_dead=None), name + ": add_mask and key_dead are both NULL (use the unmasked entry point)")
        bad(call(ldm=4), "(ldm 4, Tk 5)")
        bad(call(ldm=6), "multiple of 4 floats and >= Tk (ldm 6, Tk 5)")
        bad(call(add_mask=a4), "add_mask must be 16-byte aligned")
        bad(call(mask_stride_b=42), "mask_stride_b 42,")
        bad(call(mask_stride_h=-40), "must not be negative (mask_stride_b 0, mask_stride_h -40)")
        bad(call(mask_stride_b=-8), "must not be negative (mask_stride_b -8,")
        bad(call(ldd=4), "dead-key row stride must be >= Tk (ldd 4, Tk 5)")
        bad(call(Tq=1 << 20, ldm=1024), "one mask slice exceeds 4 GiB (Tq 1048576, ldm 1024)")
        # one mask alone is enough, and the other's stride is then not looked at: the refusal comes from a later check
        bad(call(key_dead=None, ldd=0, k=a4), name + ": q/k/v")
        bad(call(add_mask=None, ldm=0, mask_stride_b=-8, k=a4), name + ": q/k/v")
    bad(fwd(causal=1, attn=a), "attention_fwd_wide_masked: the weights are only written by the non-causal")
    bad(bwd(dq=None), "attention_bwd_wide_masked: null pointer")
    bad(bwd(lddk=128), "gradient strides must be >= H*128 = 256 (lddq 768, lddk 128,")
    bad(bwd(d_o=a4), "16-byte aligned")
    with pytest.raises(RuntimeError, match="ttts_attention_fwd_wide_masked failed"):
        _lib.check(fwd(B=0), "ttts_attention_fwd_wide_masked")


class _Count:
    """counts the device reads a mask resolution makes: torch.equal and Tensor.any"""

    def __init__(self, monkeypatch):
        self.n = 0
        equal, any_ = torch.equal, torch.Tensor.any

        def counted_equal(*a, **k):
            self.n += 1
            return equal(*a, **k)

        def counted_any(*a, **k):
            self.n += 1
            return any_(*a, **k)
        monkeypatch.setattr(torch, "equal", counted_equal)
        monkeypatch.setattr(torch.Tensor, "any", counted_any)

    def take(self):
        n, self.n = self.n, 0
        return n


def test_a_mask_tensor_is_resolved_once(monkeypatch):
    from transformertts_amd.model import layers as L
    monkeypatch.setattr(L, "_memo", L._MaskMemo())
    reads = _Count(monkeypatch)
    B, T = 2, 6
    kpm = torch.zeros(B, T, dtype=torch.bool)
    kpm[0, 2] = kpm[1, 4:] = True                       # a hole: stays a tensor
    lens, dead = L._resolve_kpm(kpm, B, T, "cpu")
    assert reads.take() >= 1 and dead is not None and lens.tolist() == [5, 4]
    assert dead is not kpm and torch.equal(dead, kpm) and reads.take() == 1      # a copy: the entry must not keep its own key alive
    again = L._resolve_kpm(kpm, B, T, "cpu")
    assert reads.take() == 0 and again[0] is lens and again[1] is dead          # the same object: no read
    kpm[1, 1] = True                                     # written in place (_version moves): resolved again
    lens2, _ = L._resolve_kpm(kpm, B, T, "cpu")
    assert reads.take() >= 1 and lens2.tolist() == [5, 3]
    L._resolve_kpm(kpm.clone(), B, T, "cpu")             # an equal but NEW tensor object misses
    assert reads.take() >= 1
    prefix = torch.arange(T)[None, :] >= torch.tensor([6, 3])[:, None]
    assert L._resolve_kpm(prefix, B, T, "cpu")[1] is None and reads.take() >= 1
    assert L._resolve_kpm(prefix, B, T, "cpu")[1] is None and reads.take() == 0

    causal = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    assert L._is_causal_mask(causal, T, T) and reads.take() == 1
    assert L._is_causal_mask(causal, T, T) and reads.take() == 0
    causal[0, 1] = False
    assert not L._is_causal_mask(causal, T, T) and reads.take() == 1
    causal_f = torch.zeros(T, T).masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    assert L._is_causal_mask(causal_f, T, T) and reads.take() >= 1
    assert L._is_causal_mask(causal_f, T, T) and reads.take() == 0

    band = torch.randn(T, T).masked_fill((torch.arange(T)[:, None] - torch.arange(T)[None, :]).abs() > 2, float("-inf"))
    m = L._additive_mask(band, B, 2, T, T)
    assert reads.take() == 1 and bool(torch.isfinite(m).all()) and m.shape == (1, 1, T, T)
    assert L._additive_mask(band, B, 2, T, T) is m and reads.take() == 0
    band[0, 0] = 1.0
    m2 = L._additive_mask(band, B, 2, T, T)
    assert m2 is not m and reads.take() == 1 and float(m2[0, 0, 0, 0]) == 1.0
    assert L._additive_mask(band.clone(), B, 2, T, T) is not m2 and reads.take() == 1
    # a tensor that died and a new one that may sit at its address: the entry is bound to the object, not the storage
    # ... and leaves with it
    for _ in range(3):
        n = len(L._memo.items)
        t = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
        assert L._is_causal_mask(t, T, T) and reads.take() == 1 and len(L._memo.items) == n + 1
        del t
        assert len(L._memo.items) == n
    holes = kpm.clone()
    L._resolve_kpm(holes, B, T, "cpu")
    n = len(L._memo.items)
    del holes
    assert len(L._memo.items) == n - 1
    # lengths AND a key-padding mask: the comparison is remembered per pair of tensor objects
    reads.take()
    lens_t = torch.tensor([6, 3])
    assert L._lens_and_kpm(lens_t, prefix, B, T, "cpu", "x") == (lens_t, None) and reads.take() == 1
    assert L._lens_and_kpm(lens_t, prefix, B, T, "cpu", "x") == (lens_t, None) and reads.take() == 0
    L._lens_and_kpm(lens_t.clone(), prefix, B, T, "cpu", "x")
    assert reads.take() == 1
    with pytest.raises(ValueError, match="not the prefix mask"):
        L._lens_and_kpm(torch.tensor([6, 2]), prefix, B, T, "cpu", "x")
    # the LRU stays small
    keep = [torch.zeros(B, T, dtype=torch.bool) for _ in range(3 * L._memo.size)]
    for t in keep:
        L._resolve_kpm(t, B, T, "cpu")
    assert len(L._memo.items) <= L._memo.size


def test_masks_have_no_cpu_path_either():
    from transformertts_amd import ops
    from transformertts_amd.model import layers as L
    dead = torch.zeros(1, 4, dtype=torch.bool)
    dead[0, 1] = True
    band = torch.zeros(4, 4).masked_fill(torch.triu(torch.ones(4, 4, dtype=torch.bool), 2), float("-inf"))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.self_attention(torch.zeros(1, 4, 3 * 64), torch.tensor([4]), 1, False, 0.0, 0, dead=dead)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.self_attention(torch.zeros(1, 4, 3 * 64), torch.tensor([4]), 1, False, 0.0, 0, add_mask=band)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.cross_attention(torch.zeros(1, 4, 96), torch.zeros(1, 4, 192), torch.tensor([4]), 1, 0.0, 0, dead=dead, add_mask=band)
    layer = L.TransformerDecoderLayer(64, 1, 128, dropout=0.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        layer(torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), memory_mask=band, memory_key_padding_mask=dead)
    # a head image or a twin batch with a mask is refused
    img = ops.HeadImage(torch.zeros(1, 4, 192), torch.zeros(1, 4), None, 64)
    with pytest.raises(ValueError, match="length masks only"):
        ops.self_attention(img, torch.tensor([4]), 1, False, 0.0, 0, dead=dead)
    with pytest.raises(ValueError, match="length masks only"):
        ops.cross_attention(ops.HeadImage(torch.zeros(1, 4, 64), torch.zeros(1, 4), None, 64), img, torch.tensor([4]), 1, 0.0, 0,
                            add_mask=band)
    full = torch.zeros(2, 4, 192)
    half = ops.twin_pair(full)[0]
    with pytest.raises(ValueError, match="length masks only"):
        ops.self_attention(half, torch.tensor([4]), 1, False, 0.0, 0, dead=dead)


# where ops.self_attention / ops.cross_attention send a call, written out from their ladders as they stood before one function
# (ops._attn_route) made the decision; one row per (caller, operands, mask tensor, weights_grad and need_weights), one letter per
# head width of _WIDTHS.  Routes: A tensor algebra, W the 128-column kernels, I the head-image kernels, H fp16x3 on 64 columns;
# refusals: the letters of _REFUSALS.
_WIDTHS = (32, 64, 96, 128, 160)
_ROUTES = {"A": "algebra", "W": "wide", "I": "image", "H": "h3"}
_REFUSALS = {"L": "{who}: a head image / twin batch takes length masks only",
             "F": "{who}: differentiable weights take fp32 operands (no head image, no twin batch)",
             "C": "{who}: head images hold 64-column heads",
             "T": "{who}: a twin batch runs on head images only"}
_ROUTE_TABLE = [
    # caller             operands  mask     weights_grad  32 .. 160
    ("self_attention",  "fp32",   "none",  False, "HHWWA"),
    ("self_attention",  "fp32",   "plain", False, "WWWWA"),
    ("self_attention",  "fp32",   "grad",  False, "AAAAA"),
    ("self_attention",  "twin",   "none",  False, "TTTTA"),      # (heads wider than 128 leave before the twin is looked at)
    ("self_attention",  "twin",   "plain", False, "LLLLL"),
    ("self_attention",  "twin",   "grad",  False, "LLLLL"),
    ("self_attention",  "image",  "none",  False, "IICCC"),
    ("self_attention",  "image",  "plain", False, "LLLLL"),
    ("self_attention",  "image",  "grad",  False, "LLLLL"),
    ("cross_attention", "fp32",   "none",  False, "HHWWA"),
    ("cross_attention", "fp32",   "plain", False, "WWWWA"),
    ("cross_attention", "fp32",   "grad",  False, "AAAAA"),
    ("cross_attention", "twin",   "none",  False, "HHWWA"),      # (the cross form never looked at the twin of an unmasked call)
    ("cross_attention", "twin",   "plain", False, "LLLLL"),
    ("cross_attention", "twin",   "grad",  False, "LLLLL"),
    ("cross_attention", "image",  "none",  False, "IICCC"),
    ("cross_attention", "image",  "plain", False, "LLLLL"),
    ("cross_attention", "image",  "grad",  False, "LLLLL"),
    ("cross_attention", "fp32",   "none",  True,  "WWWWA"),
    ("cross_attention", "fp32",   "plain", True,  "WWWWA"),
    ("cross_attention", "fp32",   "grad",  True,  "AAAAA"),
    ("cross_attention", "twin",   "none",  True,  "FFFFF"),
    ("cross_attention", "twin",   "plain", True,  "FFFFF"),
    ("cross_attention", "twin",   "grad",  True,  "FFFFF"),
    ("cross_attention", "image",  "none",  True,  "FFFFF"),
    ("cross_attention", "image",  "plain", True,  "FFFFF"),
    ("cross_attention", "image",  "grad",  True,  "FFFFF"),
]


def test_the_route_of_an_attention_call():
    from transformertts_amd import ops
    masks = {"none": None, "plain": torch.zeros(4, 4), "grad": torch.zeros(4, 4, requires_grad=True)}
    assert len({row[:4] for row in _ROUTE_TABLE}) == len(_ROUTE_TABLE) == 27
    for who, operands, mask, weights_grad, expected in _ROUTE_TABLE:
        m = masks[mask]
        for hd, letter in zip(_WIDTHS, expected, strict=True):
            args = (who, hd, operands == "image", operands == "twin", m is not None, ops._mask_needs_autograd(m), weights_grad)
            if letter in _ROUTES:
                assert ops._attn_route(*args) == _ROUTES[letter], args
            else:
                with pytest.raises(ValueError, match=re.escape(_REFUSALS[letter].format(who=who))):
                    ops._attn_route(*args)
    # ... and what the layers ask before they draw a seed is the same decision
    for hd in _WIDTHS:
        for mask in masks.values():
            assert ops.attention_on_kernels(2 * hd, 2, mask) == (hd <= 128 and not (mask is not None and mask.requires_grad))
    with torch.no_grad():       # nothing to differentiate: the mask is a plain one
        assert ops.attention_on_kernels(256, 2, masks["grad"])
