"""The 128-column attention entry points (ABI v17, csrc/attention_wide.hip): declared, exported, and their argument checks -- and
the same refusal table for the 64-column families, whose check they share.  Host logic only, no GPU (every refusal happens
before a launch)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_attention_fwd_wide", "ttts_attention_bwd_wide", "ttts_heads_pad_w", "ttts_heads_unpad_w")


def test_abi_version_and_the_header_declares_the_wide_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 17
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
    # same argument lists as the 64-column fp32 entry points (rowstat in the place of lse)
    assert _lib.SIGNATURES["ttts_attention_fwd_wide"] == _lib.SIGNATURES["ttts_attention_fwd"]
    assert _lib.SIGNATURES["ttts_attention_bwd_wide"] == _lib.SIGNATURES["ttts_attention_bwd"]
    assert len(_lib.SIGNATURES["ttts_heads_pad_w"][1]) == len(_lib.SIGNATURES["ttts_heads_pad"][1]) + 1


def test_wide_entry_points_refuse_bad_arguments_with_a_message():
    """One refusal table for every attention family (one check serves them all, csrc/attention_common.h): the 128-column entry
    points and the 64-column fp32-MFMA, bf16x6, fp16x3 and head-image ones."""
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

    def caller(fn, order, defaults):
        def call(**kw):
            unknown = set(kw) - set(order)
            assert not unknown, unknown
            return getattr(lib, fn)(*[kw.get(name, defaults.get(name)) for name in order])
        return call

    def family(suffix, fwd_extra=(), bwd_extra=(), img=False):
        scales = ["q_inv", "k_inv", "v_inv"] if img else []
        fwd = ["q", "k", "v"] + scales + ["o", "stat", "attn", "lens"] + list(dims) + list(tail) + list(fwd_extra) + ["stream"]
        bwd = (["q", "k", "v"] + scales + ["o", "d_o", "stat", "delta", "dq", "dk", "dv", "lens"] + list(dims) + list(grads) +
               list(tail) + list(bwd_extra) + ["stream"])
        ptrs = {n: a for n in ("q", "k", "v", "q_inv", "k_inv", "v_inv", "o", "d_o", "stat", "delta", "dq", "dk", "dv", "lens",
                               "q_amax", "k_amax", "v_amax", "do_amax")}
        d = dict(ptrs, **dims, **grads, **tail, q_splits=1, q_inv_rows=0, k_inv_rows=0, stat_plane=0)    # the rest: NULL
        return caller("ttts_attention_fwd" + suffix, fwd, d), caller("ttts_attention_bwd" + suffix, bwd, d)

    amax3 = ("q_amax", "k_amax", "v_amax")
    planes = ("q_inv_rows", "k_inv_rows", "stat_plane")
    # (entry-point suffix, name in the messages, columns per head, the forward requires its statistics output, callers)
    table = (("_wide", "_wide", 128, True, family("_wide")),
             ("", "", 64, False, family("")),
             ("_x6", "", 64, False, family("_x6")),
             ("_h3", "", 64, False, family("_h3", amax3 + ("o_amax_out", "rowstat_out"),
                                           ("do_amax", "dq_amax_out", "dkv_amax_out") + amax3 + ("rowstat",))),
             ("_img", "_img", 64, False, family("_img", ("v_amax", "o_amax_out", "rowstat_out") + planes,
                                                ("do_amax", "dq_amax_out", "dkv_amax_out", "dkv_partials", "q_splits") + planes,
                                                img=True)))
    for suffix, tag, w, fwd_needs_stat, (fwd, bwd) in table:
        for call, name in ((fwd, "attention_fwd" + tag), (bwd, "attention_bwd" + tag)):
            bad(call(q=None), name + ": null pointer")
            if fwd_needs_stat or call is bwd:
                bad(call(stat=None), name + ": null pointer")
            bad(call(lens=None), name + ": null pointer")
            bad(call(B=0), "sizes must be positive (B 0,")
            bad(call(H=-1), "H -1,")
            bad(call(Tq=0), "Tq 0,")
            bad(call(Tk=0), "Tk 0)")
            bad(call(ldq=770), "multiples of 4 floats (ldq 770,")
            bad(call(ldv=769), "ldv 769,")
            bad(call(ldo=258), "ldo 258)")
            bad(call(ldk=w), f">= H*{w} = {2 * w} (ldq 768, ldk {w},")
            bad(call(p=1.0), "dropout p 1 is outside [0, 1)")
            bad(call(p=-0.25), "dropout p -0.25 is outside [0, 1)")
            bad(call(p=float("nan")), "is outside [0, 1)")
            bad(call(causal=1, Tk=6), "causal form needs Tq == Tk (Tq 5, Tk 6)")
            bad(call(k=a4), "16-byte aligned")
            assert name + ":" in _lib.last_error(), (suffix, _lib.last_error())
        bad(fwd(causal=1, attn=a), "non-causal")
        bad(bwd(dq=None), "null pointer")
        bad(bwd(lddk=w), f"gradient strides must be >= H*{w} = {2 * w} (lddq 768, lddk {w},")
        bad(bwd(d_o=a4), "16-byte aligned")
    fwd = table[0][4][0]
    # the head-image entry points keep their own checks on top
    img_fwd, img_bwd = table[4][4]
    bad(img_fwd(v_amax=None), "attention_fwd_img: null pointer")
    bad(img_bwd(do_amax=None), "attention_bwd_img: null pointer")
    bad(img_fwd(B=4, Tq=300, Tk=300, q_inv_rows=1199), "plane strides smaller than the batch")
    bad(img_bwd(stat_plane=9), "plane strides smaller than the batch")
    bad(img_fwd(Tq=1 << 20, ldq=1024), "exceeds 4 GiB")
    bad(img_bwd(Tq=1 << 20, ldo=1024), "d_o exceeds 4 GiB")
    bad(img_bwd(q_splits=17), "q_splits out of 1..16")
    bad(img_bwd(q_splits=2), "query splits need a workspace")
    # ... and the fp16x3 ones the partial maxima of their operands
    bad(table[3][4][0](q_amax=None), "q_amax / k_amax / v_amax are required")
    bad(table[3][4][1](do_amax=None), "do_amax, q_amax, k_amax and v_amax")

    # ttts_heads_pad_w(src, ld_src, dst, rows, H, head_dim, width, stream) / ttts_heads_unpad_w(src, dst, ld_dst, rows, H, ...)
    bad(lib.ttts_heads_pad_w(a, 192, a, 4, 2, 96, 96, None), "width 96 must be 64 or 128")
    bad(lib.ttts_heads_unpad_w(a, a, 192, 4, 2, 96, 256, None), "width 256 must be 64 or 128")
    bad(lib.ttts_heads_pad_w(a, 192, a, 4, 2, 96, 64, None), "head_dim 96 must be in 1..64")      # the 64-column form, unchanged
    bad(lib.ttts_heads_pad_w(a, 192, a, 4, 2, 129, 128, None), "head_dim 129 must be in 1..128")
    bad(lib.ttts_heads_pad_w(None, 192, a, 4, 2, 96, 128, None), "heads_pad_w: bad arguments")
    bad(lib.ttts_heads_pad_w(a, 100, a, 4, 2, 96, 128, None), "heads_pad_w: bad arguments")       # ld_src < H * head_dim
    bad(lib.ttts_heads_unpad_w(a, a, 192, 0, 2, 96, 128, None), "heads_unpad_w: bad arguments")
    with pytest.raises(RuntimeError, match="ttts_attention_fwd_wide failed"):
        _lib.check(fwd(B=0), "ttts_attention_fwd_wide")


def test_wide_heads_have_no_cpu_path_either():
    import torch
    from transformertts_amd import ops
    assert ops._head_width(1024, 8) == 128
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.self_attention(torch.zeros(1, 4, 3 * 128), torch.tensor([4]), 1, True, 0.0, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.cross_attention(torch.zeros(1, 4, 96), torch.zeros(1, 3, 192), torch.tensor([3]), 1, 0.0, 0)
