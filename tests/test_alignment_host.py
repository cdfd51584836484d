"""Phoneme durations from the alignment maps (ABI v20, csrc/alignment.hip; transformertts_amd/alignment.py): the entry points are
declared, bound and exported, ctypes and the header agree, every refusal comes with its message before any launch, the workspace
query, and the argument refusals of `extract_durations`.  Host logic only, no GPU."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttts_alignment_rowstats", "ttts_alignment_select", "ttts_alignment_durations_argmax", "ttts_alignment_mas",
       "ttts_alignment_mas_workspace_bytes")


def test_abi_version_and_the_header_declares_the_new_entry_points():
    from transformertts_amd import _lib
    lib = _lib.load()
    assert lib.ttts_abi_version() >= 20
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in ttts_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not exported / bound"
        decl = re.search(r"^(?:int|size_t) " + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name      # ctypes and the header agree on the argument count
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[NEW[0]] == (I, [P, L, L, L, P, P, I, I, I, I, I, I, P, P, P, P])
    assert _lib.SIGNATURES[NEW[3]] == (I, [P, I, L, L, L, P, P, P, I, I, I, I, P, Z, P, P, P])
    assert _lib.SIGNATURES[NEW[4]] == (Z, [I, I, I])
    # the block states what it replaces and the definitions
    block = hdr[hdr.index("ABI v20; alignment.hip"):hdr.index("int ttts_alignment_rowstats")]
    for needle in ("attn.max(-1)", ".argmax(-1)", "torch.bincount", "output['alignments']", "model/layers.py:68-74",
                   "(1 / T_b) sum_{t < T_b} max_n A[t][n]", "logf(fmaxf(A[t][n], 1e-30f))", "Q[t-1][n] >= Q[t-1][n-1]", "T_b < N_b"):
        assert needle in block, needle
    assert [int(re.search(rf"#define TTTS_ALIGN_SELECT_{m} (\d+)", hdr).group(1)) for m in ("UTTERANCE", "BATCH", "FIXED")] == [0, 1, 2]
    from transformertts_amd import alignment
    assert alignment.SELECT_MODES == {"utterance": 0, "batch": 1}
    assert alignment.MAX_MAPS == int(re.search(r"#define TTTS_ALIGN_MAX_MAPS (\d+)", hdr).group(1)) == 16


def test_entry_points_refuse_bad_arguments_with_a_message():
    from transformertts_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # a 16-byte aligned host address (never dereferenced)
    a4 = ctypes.c_void_p(a.value + 4)

    def bad(rc, needle):
        assert rc == -1, rc
        assert needle in _lib.last_error(), _lib.last_error()

    def caller(fn, names, defaults):
        def call(**kw):
            assert not set(kw) - set(names)
            return fn(*[kw.get(n, defaults[n]) for n in names])
        return call

    sizes = dict(B=2, H=4, Tm=7, Tp=5)
    rn = ["attn", "ld_row", "ld_head", "ld_batch", "plens", "mlens", "B", "H", "Tm", "Tp", "layer", "L", "argmax", "rowmax", "focus",
          "stream"]
    rows = caller(lib.ttts_alignment_rowstats, rn, dict(sizes, attn=a, ld_row=5, ld_head=35, ld_batch=140, plens=a, mlens=a, layer=0,
                                                       L=2, argmax=a, rowmax=a, focus=a, stream=None))
    e = "alignment_rowstats"
    for p in ("attn", "plens", "mlens", "argmax", "rowmax", "focus"):
        bad(rows(**{p: None}), e + ": null pointer")
    bad(rows(Tp=0, ld_row=0), e + ": sizes must be positive (B 2, H 4, Tm 7, Tp 0)")
    bad(rows(B=-1), e + ": sizes must be positive (B -1,")
    bad(rows(L=0), e + ": sizes must be positive (L 0)")
    bad(rows(L=17), e + ": at most 16 maps (L 17)")
    bad(rows(layer=2), e + ": layer 2 is outside [0, L 2)")
    bad(rows(layer=-1), e + ": layer -1 is outside [0, L 2)")
    bad(rows(ld_row=4), e + ": the row stride must be >= Tp (ld_row 4, Tp 5)")
    bad(rows(ld_head=-35), e + ": strides must not be negative (ld_head -35, ld_batch 140)")
    bad(rows(B=1 << 16, H=1 << 8, Tm=1 << 7), e + ": grid too large (B*H*Tm 2147483648)")

    sn = ["focus", "plens", "mlens", "L", "B", "H", "mode", "layer", "head", "choice", "pairs", "stream"]
    sel = caller(lib.ttts_alignment_select, sn, dict(focus=a, plens=a, mlens=a, L=3, B=2, H=4, mode=0, layer=0, head=0, choice=a,
                                                     pairs=None, stream=None))
    e = "alignment_select"
    for p in ("focus", "plens", "mlens", "choice"):
        bad(sel(**{p: None}), e + ": null pointer")
    bad(sel(H=0), e + ": sizes must be positive (B 2, H 0)")
    bad(sel(L=0), e + ": sizes must be positive (L 0)")
    bad(sel(L=17), e + ": at most 16 maps (L 17)")
    bad(sel(mode=3), e + ": unknown mode 3")
    bad(sel(mode=-1), e + ": unknown mode -1")
    bad(sel(mode=2, layer=3), e + ": (layer 3, head 0) is outside (L 3, H 4)")
    bad(sel(mode=2, head=4), e + ": (layer 0, head 4) is outside (L 3, H 4)")
    bad(sel(mode=2, head=-1), e + ": (layer 0, head -1) is outside (L 3, H 4)")
    bad(sel(L=16, H=65), e + ": at most 1024 (layer, head) pairs (L*H 1040)")

    dn = ["argmax", "choice", "plens", "mlens", "L", "B", "H", "Tm", "Tp", "dur", "valid", "stream"]
    cnt = caller(lib.ttts_alignment_durations_argmax, dn, dict(sizes, argmax=a, choice=a, plens=a, mlens=a, L=2, dur=a, valid=None,
                                                               stream=None))
    e = "alignment_durations_argmax"
    for p in ("argmax", "choice", "plens", "mlens", "dur"):
        bad(cnt(**{p: None}), e + ": null pointer")
    bad(cnt(Tm=0), e + ": sizes must be positive (B 2, H 4, Tm 0, Tp 5)")
    bad(cnt(L=17), e + ": at most 16 maps (L 17)")
    bad(cnt(Tp=4097), e + ": Tp 4097 is above the 4096 phonemes the counters hold")

    maps = (ctypes.c_void_p * 17)(*[a.value] * 17)
    holed = (ctypes.c_void_p * 3)(a.value, None, a.value)
    need = lib.ttts_alignment_mas_workspace_bytes(2, 7, 5)
    mn = ["maps", "L", "ld_row", "ld_head", "ld_batch", "choice", "plens", "mlens", "B", "H", "Tm", "Tp", "ws", "ws_bytes", "dur",
          "valid", "stream"]
    mas = caller(lib.ttts_alignment_mas, mn, dict(sizes, maps=maps, L=3, ld_row=8, ld_head=56, ld_batch=224, choice=a, plens=a, mlens=a,
                                                  ws=a, ws_bytes=need, dur=a, valid=a, stream=None))
    e = "alignment_mas"
    for p in ("maps", "choice", "plens", "mlens", "ws", "dur", "valid"):
        bad(mas(**{p: None}), e + ": null pointer")
    bad(mas(maps=holed), e + ": null pointer (map 1)")
    bad(mas(H=0), e + ": sizes must be positive (B 2, H 0, Tm 7, Tp 5)")
    bad(mas(L=0), e + ": sizes must be positive (L 0)")
    bad(mas(L=17), e + ": at most 16 maps (L 17)")
    bad(mas(ld_row=4), e + ": the row stride must be >= Tp (ld_row 4, Tp 5)")
    bad(mas(ld_batch=-1), e + ": strides must not be negative (ld_head 56, ld_batch -1)")
    bad(mas(Tp=1025, ld_row=1025, ws_bytes=1 << 30), e + ": Tp 1025 is above the 1024 phonemes one wave holds")
    bad(mas(ws=a4), e + ": the workspace must be 8-byte aligned")
    bad(mas(ws_bytes=need - 1), e + f": workspace too small ({need - 1} bytes, {need} needed)")
    bad(mas(ws_bytes=0), e + f": workspace too small (0 bytes, {need} needed)")


def test_mas_workspace_query_is_positive_and_monotonic():
    from transformertts_amd import _lib
    q = _lib.load().ttts_alignment_mas_workspace_bytes
    assert q(1, 1, 1) == 8                                           # one 64-bit word of stay bits per (utterance, frame)
    assert q(64, 870, 160) == 64 * 870 * 4 * 8                       # 160 phonemes: four per lane
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5)):
        assert q(*bad) == 0
    grid = [(B, Tm, Tp) for B in (1, 2, 5, 64) for Tm in (1, 2, 150, 870, 3001) for Tp in (1, 13, 64, 65, 70, 128, 129, 130, 256, 257,
                                                                                         512, 513, 1024)]
    for B, Tm, Tp in grid:
        v = q(B, Tm, Tp)
        assert v > 0 and v % 8 == 0 and v * 8 >= B * Tm * Tp         # at least one bit per cell
        assert q(B + 1, Tm, Tp) > v and q(B, Tm + 1, Tp) > v and q(B, Tm, Tp + 1) >= v


def test_extract_durations_refuses_bad_arguments():
    import transformertts_amd
    from transformertts_amd.alignment import extract_durations, teacher_durations
    assert transformertts_amd.extract_durations is extract_durations and transformertts_amd.teacher_durations is teacher_durations
    maps, pl, ml = [torch.zeros(2, 4, 6, 5)] * 3, torch.tensor([5, 3]), torch.tensor([6, 4])
    with pytest.raises(ValueError, match="method must be one of"):
        extract_durations(maps, pl, ml, method="viterbi")
    with pytest.raises(ValueError, match="select must be 'utterance', 'batch' or \\(layer, head\\)"):
        extract_durations(maps, pl, ml, select="best")
    with pytest.raises(ValueError, match="select must be 'utterance', 'batch' or \\(layer, head\\)"):
        extract_durations(maps, pl, ml, select=(1, 2, 3))
    with pytest.raises(ValueError, match="select must be 'utterance', 'batch' or \\(layer, head\\)"):
        extract_durations(maps, pl, ml, select=1)
    with pytest.raises(ValueError, match="\\(layer 3, head 0\\) of 3 maps with 4 heads"):
        extract_durations(maps, pl, ml, select=(3, 0))
    with pytest.raises(ValueError, match="\\(layer 0, head 4\\) of 3 maps with 4 heads"):
        extract_durations(maps, pl, ml, select=(0, 4))
    with pytest.raises(ValueError, match="no alignment maps"):
        extract_durations([], pl, ml)
    with pytest.raises(ValueError, match="an alignment map is None"):
        extract_durations([maps[0], None], pl, ml)
    with pytest.raises(ValueError, match="at most 16 alignment maps, got 17"):
        extract_durations([maps[0]] * 17, pl, ml)
    with pytest.raises(ValueError, match="maps differ in shape"):
        extract_durations([maps[0], torch.zeros(2, 4, 6, 4)], pl, ml)
    with pytest.raises(ValueError, match="alignment maps are \\(B, H, Tm, Tp\\)"):
        extract_durations([torch.zeros(2, 6, 5)], pl, ml)
    with pytest.raises(ValueError, match="phoneme_lens must have shape \\(2,\\), got \\(3,\\)"):
        extract_durations(maps, torch.tensor([5, 3, 1]), ml)
    with pytest.raises(ValueError, match="mel_lens must have shape \\(2,\\), got \\(2, 1\\)"):
        extract_durations(maps, pl, ml[:, None])
    with pytest.raises(ValueError, match="mel_lens must be integers"):
        extract_durations(maps, pl, ml.float())
    for method in ("mas", "argmax"):
        with pytest.raises(ValueError, match="no CPU fallback"):      # HIP tensors only
            extract_durations(maps, pl, ml, method=method, select=(2, 3))


def test_which_map_layouts_are_read_in_place():
    """`alignment._strides` / `_operands` on CPU tensors (they read shapes and strides only)"""
    from transformertts_amd.alignment import _operands, _strides
    B, H, Tm, Tp = 2, 3, 5, 7
    assert _strides(torch.zeros(B, H, Tm, Tp)) == (Tp, Tm * Tp, H * Tm * Tp)
    assert _strides(torch.zeros(B, H, Tm, 8)[..., :Tp]) == (8, Tm * 8, H * Tm * 8)           # padded rows: a view, in place
    assert _strides(torch.zeros(B, 1, Tm, Tp).expand(B, H, Tm, Tp)) == (Tp, 0, Tm * Tp)      # expanded over the heads
    assert _strides(torch.zeros(B, H, Tm, 12)[..., 1:8]) == (12, Tm * 12, H * Tm * 12)       # no alignment is asked
    assert _strides(torch.zeros(B, H, Tp, Tm).transpose(2, 3)) is None                       # columns not contiguous
    assert _strides(torch.zeros(B, H, Tm, 2 * Tp)[..., ::2]) is None
    assert _strides(torch.zeros(1, 1, 1, Tp)) == (Tp, 0, 0)
    view = torch.zeros(B, H, Tm, 8)[..., :Tp]
    ops_, st = _operands([view, view.clone(memory_format=torch.preserve_format)])
    assert len({m.stride() for m in ops_}) == 1 and st == _strides(ops_[0])                  # one set of strides for all maps
    same, st = _operands([view, view])
    assert same[0].data_ptr() == view.data_ptr() and st == (8, Tm * 8, H * Tm * 8)           # ... and no copy when they agree
    t, _ = _operands([torch.zeros(B, H, Tp, Tm).transpose(2, 3)])
    assert t[0].is_contiguous()


def test_the_benchmarks_stock_torch_side_is_the_extraction():
    """tools/durations_bench.py times the kernels against `torch_argmax` / `torch_mas`; those are the same extraction: on CPU
    tensors they agree with `bincount` of `argmax` and with the fp64 dynamic programme of tests/test_hip_alignment.py, an
    utterance with T < N included"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import durations_bench as bench
    finally:
        sys.path.pop(0)
    from test_hip_alignment import _first_max, _mas64
    Lm, B, H, Tm, Tp = 2, 6, 3, 40, 17
    maps, plens, mlens = bench.make_case(Lm, B, H, Tm, Tp, torch.device("cpu"), seed=3)
    plens[3], mlens[3] = 9, 5
    dur_m, focus, choice = bench.torch_mas(maps, plens, mlens, plens, mlens)
    dur_a, focus_a, choice_a = bench.torch_argmax(maps, plens, mlens, plens, mlens)
    assert torch.equal(choice, choice_a) and torch.equal(focus, focus_a)
    pairs = _first_max(focus)
    assert torch.equal(pairs[:, 0] * H + pairs[:, 1], choice) and len(set(choice.tolist())) > 1
    for b in range(B):
        T, N = int(mlens[b]), int(plens[b])
        plane = maps[int(pairs[b, 0])][b, int(pairs[b, 1])]
        assert abs(float(focus[int(pairs[b, 0]), b, int(pairs[b, 1])]) - float(plane[:T].max(-1).values.double().mean())) < 1e-6
        assert torch.equal(dur_a[b], torch.bincount(plane[:T].argmax(-1), minlength=Tp))
        if T < N:
            assert int(dur_m[b].abs().sum()) == 0
        else:
            assert torch.equal(dur_m[b, :N], _mas64(plane, T, N)[0]) and int(dur_m[b].sum()) == T
