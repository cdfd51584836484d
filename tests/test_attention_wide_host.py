"""The 128-column attention entry points (ABI v17, csrc/attention_wide.hip): declared, exported, and their argument checks --
host logic only, no GPU (every refusal happens before a launch)."""
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
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a4 = ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    def fwd(q=a, k=a, v=a, o=a, rowstat=a, attn=None, lens=a, B=1, H=2, Tq=5, Tk=5, ldq=768, ldk=768, ldv=768, ldo=256,
            causal=0, scale=0.1, p=0.0):
        return lib.ttts_attention_fwd_wide(q, k, v, o, rowstat, attn, lens, B, H, Tq, Tk, ldq, ldk, ldv, ldo, causal, scale, p,
                                           0, None, None)

    def bwd(q=a, k=a, v=a, o=a, d_o=a, rowstat=a, delta=a, dq=a, dk=a, dv=a, lens=a, B=1, H=2, Tq=5, Tk=5, ldq=768, ldk=768,
            ldv=768, ldo=256, lddq=768, lddk=768, lddv=768, causal=0, scale=0.1, p=0.0):
        return lib.ttts_attention_bwd_wide(q, k, v, o, d_o, rowstat, delta, dq, dk, dv, lens, B, H, Tq, Tk, ldq, ldk, ldv, ldo,
                                           lddq, lddk, lddv, causal, scale, p, 0, None, None)

    for call, name in ((fwd, "attention_fwd_wide"), (bwd, "attention_bwd_wide")):
        bad(call(q=None), name + ": null pointer")
        bad(call(rowstat=None), name + ": null pointer")
        bad(call(lens=None), name + ": null pointer")
        bad(call(B=0), "sizes must be positive (B 0,")
        bad(call(H=-1), "H -1,")
        bad(call(Tq=0), "Tq 0,")
        bad(call(Tk=0), "Tk 0)")
        bad(call(ldq=770), "multiples of 4 floats (ldq 770,")
        bad(call(ldv=769), "ldv 769,")
        bad(call(ldo=258), "ldo 258)")
        bad(call(ldk=128), ">= H*128 = 256 (ldq 768, ldk 128,")
        bad(call(p=1.0), "dropout p 1 is outside [0, 1)")
        bad(call(p=-0.25), "dropout p -0.25 is outside [0, 1)")
        bad(call(p=float("nan")), "is outside [0, 1)")
        bad(call(causal=1, Tk=6), "causal form needs Tq == Tk (Tq 5, Tk 6)")
        bad(call(k=a4), "16-byte aligned")
    bad(fwd(causal=1, attn=a), "non-causal")
    bad(bwd(dq=None), "null pointer")
    bad(bwd(lddk=128), "gradient strides must be >= H*128 = 256 (lddq 768, lddk 128,")
    bad(bwd(d_o=a4), "16-byte aligned")

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
