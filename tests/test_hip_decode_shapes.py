"""The decode kernels (csrc/decode.hip) and the Synthesizer at the widths they ship at and on every dispatch branch: the GEMV
over its whole (K chunks, columns per wave) matrix, LayerNorm over its width range, attention at the head dims 48 / 80 / 96 / 112
and at B = 64 with lengths on every edge, the stop decision past row 15 (the second and later passes of decode_stop_kernel),
the engine at B = 17 / 20 / 64, at the capacity and key-block roundings and at the advertised size limits.

Every kernel-level output sits in a sentinel-filled buffer with guard rows behind it (conftest.guarded); references are fp64.

Which case runs which instantiation (KC = ceil(K / 256) rounded up to 1, 2, 4, 8, 16; NC = 1 below M = 8, else 4, 4, 4, 2, 1):
  decode_linear_kernel<1,1> <1,4>    test_decode_linear_dispatch[4|80|252|256], M < 8 / M >= 8
  decode_linear_kernel<2,1> <2,4>    test_decode_linear_dispatch[260|512]
  decode_linear_kernel<4,1> <4,4>    test_decode_linear_dispatch[1024]
  decode_linear_kernel<8,1> <8,2>    test_decode_linear_dispatch[1028|2048]; in the engine test_scaled_b9_vs_fp64_oracle (<8,2>)
  decode_linear_kernel<16,1>         test_decode_linear_dispatch[2052|4096] (both row ranges); in the engine test_wide_config_vs_fp64_oracle
  decode_attn_*<48|80|96|112, false> test_decode_attention_untested_head_dims
  decode_attn_*<48|80|96|112, true>  test_decode_attention_edges[hd-...] (map-writing), and <64,*>, <128,*> there as well
  decode_stop_kernel<1|2|4|8>        test_frame_out_vs_fp64 / test_frame_out_stop_decision_past_row_15 (d = 256 .. 2048)
"""
from ctypes import c_void_p

import pytest
import torch

import test_hip_synthesis as S1
import test_hip_synthesis_ragged as S2
from conftest import guarded, rel_l2
from test_hip_synthesis import _attn_ref, _batch, _build, _lib_stream, _p
from test_hip_synthesis_ragged import (_assert_zero_behind, _first_crossings, _fit_stop_head, _oracle64, _oracle_alignments, _ramps,
                                       GATE, KERNEL_GATE, KEYS, MARGIN, PATH_GATE, PER_ROW, SENT)

pytestmark = pytest.mark.gpu
NAN = float("nan")

# Hard LayerNorm rows (mean 1e3, unit spread; _hard_ln_inputs).  The gate is 4 x the rel-L2 of torch.nn.functional.layer_norm
# in fp32 on the CPU against fp64 on the same inputs (the margin: a different, equally valid summation order).
#   d = 256:  CPU fp32 2.696e-05, the kernel 1.890e-05
#   d = 1024: CPU fp32 2.168e-05, the kernel 1.971e-05
HARD_LN_CPU = {256: 2.696e-05, 1024: 2.168e-05}
# One-hot attention (q x 30, the largest score moved into the last / the first key block; _onehot_inputs).  The gate is 4 x the
# rel-L2 of the same softmax-attention evaluated in fp32 on the CPU (_attn_ref32) against fp64 on the same inputs (the figure
# depends on the CPU's BLAS: another host gave 1.112e-06 / 9.639e-07; the smaller pair is the gate).
#   last:  CPU fp32 7.031e-07, the kernel 6.555e-07
#   first: CPU fp32 7.419e-07, the kernel 6.558e-07
ONEHOT_CPU = {"last": 7.031e-07, "first": 7.419e-07}


def _rows_state(t, row_end, **kw):
    return S2._state(t, row_end, **kw)


def _i64(t):
    return c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ A1: the GEMV
K_ALL = [4, 80, 252, 256, 260, 512, 1024, 1028, 2048, 2052, 4096]
M_ALL = [1, 4, 7, 8, 9, 17, 64, 65]
N_ALL = [1, 3, 5, 15, 17, 80, 1027]
COMBOS = [(act, bias, res) for act in (0, 1) for bias in (False, True) for res in (False, True)]


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(700)
    return dict(w=torch.randn(1027, 4096, generator=g), x=torch.randn(65, 4096, generator=g),
                b=torch.randn(1027, generator=g), r=torch.randn(65, 1027, generator=g))


def _lin_operands(pool, M, N, K):
    x = pool["x"][:M, :K].contiguous()
    w = (pool["w"][:N, :K] / K ** 0.5).contiguous()
    return x, w, pool["b"][:N].contiguous(), pool["r"][:M, :N].contiguous()


def _lin_want(x, w, b, r, act, bias, res):
    want = x.double() @ w.double().T
    if bias:
        want = want + b.double()
    if act:
        want = want.clamp_min(0)
    if res:
        want = want + r.double()
    return want


def _padded(x, ld, fill):
    """(M, ld) on the device: x in the leading columns, `fill` behind them"""
    buf = torch.full((x.shape[0], ld), fill, dtype=torch.float32)
    buf[:, :x.shape[1]] = x
    return buf.cuda()


def _one_sign(x, w):
    """operands whose products all have one sign within a column (positive in the even columns, negative in the odd ones):
    every dot product has condition number 1, whatever the size of the output"""
    sign = torch.where(torch.arange(w.shape[0]) % 2 == 0, 1.0, -1.0).unsqueeze(1)
    return x.abs() + 0.5, (w.abs() + 0.5 / w.shape[1] ** 0.5) * sign


@pytest.mark.parametrize("K", K_ALL)
def test_decode_linear_dispatch(K, pool):
    """every (K, M, N) of the dispatch matrix, the activation / bias / residual combinations rotating over it; x rows ldx = K + 4
    apart with NaN behind each (finite result, bitwise the one with finite padding), the residual ldr = N + 3 apart, the output
    ldy = N + 5 apart with the sentinel kept behind each row and in the guard rows.

    Two sets of operands.  "one sign": no cancellation inside a dot product, and a product large against the bias and the
    residual, so the relative error of an output is the kernel's own and the gate means the same for one output element as
    for 65 x 1027; every case runs on it.  "zero mean": the plain normal operands of test_decode_linear_vs_fp64, whose terms
    cancel.  Over many outputs that is the sharper probe of the summation; over one it measures the draw: at K = 4096,
    M = N = 1 the dot product 1.0679 meets the bias -1.0962, the kernel's error of 1.2e-7 (one ulp of the dot product)
    becomes 4.1e-6 of the result, and at K = 512 relu(0.7425) + residual -0.8043 turns 7e-8 into 1.15e-6.  So every case with
    at least 16 output elements, where the norm of the output is a stable denominator, runs on these operands as well."""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    st = S1._state(1)
    seen = set()
    for iN, N in enumerate(N_ALL):
        x0, w0, b, r = _lin_operands(pool, 65, N, K)
        bd = b.cuda()
        rd = _padded(r, N + 3, NAN)
        for kind, (x, w) in (("one sign", _one_sign(x0, w0)), ("zero mean", (x0, w0))):
            wd = w.contiguous().cuda()
            xn, xf = _padded(x, K + 4, NAN), _padded(x, K + 4, 3.0)
            for iM, M in enumerate(M_ALL):
                if kind == "zero mean" and M * N < 16:
                    continue
                act, bias, res = COMBOS[(iN + 3 * iM + K_ALL.index(K)) % 8]
                seen.add((act, bias, res))
                want = _lin_want(x[:M], w, b, r[:M], act, bias, res)
                outs = []
                for xd in (xn, xf):
                    y, chk = guarded((M, N + 5), SENT)
                    _lib.check(lib.ttts_decode_linear(_p(xd), K + 4, 0, _p(wd), _p(bd) if bias else None,
                                                      _p(rd) if res else None, N + 3, _p(y), N + 5, 0, None, 0, 0, N, M, N, K, act,
                                                      _p(st), s), "ttts_decode_linear")
                    torch.cuda.synchronize()
                    chk()
                    assert bool((y[:, N:] == SENT).all()), (kind, K, M, N)
                    outs.append(y[:, :N].clone())
                assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1]), (kind, K, M, N)
                e = rel_l2(outs[0], want)
                assert e <= KERNEL_GATE, (kind, K, M, N, act, bias, res, e)
    assert len(seen) == 8


@pytest.mark.parametrize("K,M", [(256, 4), (256, 9), (2048, 4), (2048, 9), (4096, 7), (4096, 8)])
def test_decode_linear_split_inside_a_column_group(K, M, pool):
    """N = 17 split after column 5 (not a multiple of 4: the split falls inside one wave's columns where a wave holds several):
    both destinations against fp64, and nothing else of either is touched"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    N, ns = 17, 5
    st = S1._state(1)
    x, w, b, r = _lin_operands(pool, M, N, K)
    want = _lin_want(x, w, b, r, 0, True, False)
    y, chk = guarded((M, ns + 2), SENT)
    y2, chk2 = guarded((M, N - ns + 3), SENT)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    _lib.check(lib.ttts_decode_linear(_p(xd), K, 0, _p(wd), _p(bd), None, 0, _p(y), ns + 2, 0, _p(y2), N - ns + 3, 0, ns, M, N, K,
                                      0, _p(st), s), "ttts_decode_linear")
    torch.cuda.synchronize()
    chk()
    chk2()
    assert bool((y[:, ns:] == SENT).all()) and bool((y2[:, N - ns:] == SENT).all())
    assert rel_l2(y[:, :ns], want[:, :ns]) <= KERNEL_GATE
    assert rel_l2(y2[:, :N - ns], want[:, ns:]) <= KERNEL_GATE


# 21 rows = five workgroups of four and one of one.  First pattern: an ended row in each of the four positions of a workgroup
# (0, 5, 14, 19), a whole workgroup ended (8 .. 11) and the last, partial one ended; second: the partial one running next to
# a whole ended workgroup
ROWS_21 = [[5 if m in (0, 5, 8, 9, 10, 11, 14, 19, 20) else (-1 if m % 2 else 0) for m in range(21)],
           [3 if m in (1, 6, 15, 16, 17, 18, 19) else -1 for m in range(21)]]


@pytest.mark.parametrize("K,N", [(256, 17), (2048, 80), (4096, 17), (1024, 1027)])
def test_decode_linear_rows_21(K, N, pool):
    """running rows are bitwise what they are with no row ended (and that is fp64's at the kernel gate), ended rows keep the
    sentinel"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    M = 21
    x, w, b, r = _lin_operands(pool, M, N, K)
    want = _lin_want(x, w, b, r, 1, True, True)
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), r.cuda()

    def run(row_end):
        st = _rows_state(1, row_end)
        y, chk = guarded((M, N), SENT)
        _lib.check(lib.ttts_decode_linear_rows(_p(xd), K, 0, _p(wd), _p(bd), _p(rd), N, _p(y), N, 0, None, 0, 0, N, M, N, K, 1,
                                               _p(st, 8), _p(st), s), "ttts_decode_linear_rows")
        torch.cuda.synchronize()
        chk()
        assert st.cpu()[4:].tolist() == list(row_end) + [1] * (-M % 4)      # row state is only read
        return y

    ref = run([-1] * M)
    assert rel_l2(ref, want) <= KERNEL_GATE
    for pattern in ROWS_21:
        y = run(pattern)
        for m in range(M):
            if pattern[m] > 0:
                assert bool((y[m] == SENT).all()), (K, N, m)
            else:
                assert torch.equal(y[m], ref[m]), (K, N, m)


# ------------------------------------------------------------------------------------------------ A2: LayerNorm
@pytest.mark.parametrize("d", [1, 16, 63, 64, 65, 256, 1000, 1024])
def test_decode_layernorm_widths(d):
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(800 + d)
    st = S1._state(1)
    gam, bet = torch.randn(d, generator=g), torch.randn(d, generator=g)
    gd, bd = gam.cuda(), bet.cuda()
    for M in (1, 3, 4, 5, 64):
        x = torch.randn(M, d, generator=g) * 3 + 1
        xd = x.cuda()
        want = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-5)
        y, chk = guarded((M, d), NAN)
        _lib.check(lib.ttts_decode_layernorm(_p(xd), _p(gd), _p(bd), _p(y), M, d, 1e-5, _p(st), s), "ttts_decode_layernorm")
        torch.cuda.synchronize()
        chk()
        e = rel_l2(y, want)
        assert e <= KERNEL_GATE, (d, M, e)
        # per-row state: ended rows in the first and the last (partial) workgroup keep the sentinel, the others are bitwise equal
        ended = {m for m in (1, 4, M - 1) if 0 <= m < M and M > 1}
        row_end = [9 if m in ended else -1 for m in range(M)]
        rs = _rows_state(1, row_end)
        y2, chk2 = guarded((M, d), SENT)
        _lib.check(lib.ttts_decode_layernorm_rows(_p(xd), _p(gd), _p(bd), _p(y2), M, d, 1e-5, _p(rs, 8), _p(rs), s),
                   "ttts_decode_layernorm_rows")
        torch.cuda.synchronize()
        chk2()
        for m in range(M):
            if m in ended:
                assert bool((y2[m] == SENT).all()), (d, M, m)
            else:
                assert torch.equal(y2[m], y[m]), (d, M, m)


def _hard_ln_inputs(d):
    g = torch.Generator().manual_seed(900 + d)
    x = 1000.0 + torch.randn(64, d, generator=g)
    return x, torch.randn(d, generator=g), torch.randn(d, generator=g)


@pytest.mark.parametrize("d", [256, 1024])
def test_decode_layernorm_large_mean(d):
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    x, gam, bet = _hard_ln_inputs(d)
    want = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-5)
    cpu = rel_l2(torch.nn.functional.layer_norm(x, (d,), gam, bet, 1e-5), want)
    st = S1._state(1)
    xd, gd, bd = x.cuda(), gam.cuda(), bet.cuda()
    y, chk = guarded((64, d), NAN)
    _lib.check(lib.ttts_decode_layernorm(_p(xd), _p(gd), _p(bd), _p(y), 64, d, 1e-5, _p(st), s), "ttts_decode_layernorm")
    torch.cuda.synchronize()
    chk()
    e = rel_l2(y, want)
    print(f"layernorm, mean 1e3, d = {d}: fp32 on this CPU {cpu:.3e} (recorded {HARD_LN_CPU[d]:.3e}), the kernel {e:.3e}")
    assert e <= 4 * HARD_LN_CPU[d], (d, e, HARD_LN_CPU[d])


# ------------------------------------------------------------------------------------------------ A3: attention
@pytest.mark.parametrize("hd", [48, 80, 96, 112])
def test_decode_attention_untested_head_dims(hd):
    """the checks of test_decode_attention_vs_fp64 (self-attention at t = 1 .. 1499, ragged cross-attention, NaN past the
    length) at the head dims that test leaves out; H = 256 // hd heads"""
    S1.test_decode_attention_vs_fp64(hd)


def _edge_lens(B, max_keys):
    special = [0, 1, 63, 64, 65, max_keys, max_keys + 9]
    return torch.tensor([special[b] if b < len(special) else (b * 37) % (max_keys + 10) for b in range(B)], dtype=torch.int64)


def _softmax_rows(q, k, L, H, hd):
    """fp64 (H, L) attention weights of one utterance"""
    qh = q.double().view(H, hd) / hd ** 0.5
    kh = k[:L].double().view(L, H, hd).transpose(0, 1)
    return torch.softmax(torch.einsum("hd,hkd->hk", qh, kh), dim=-1)


@pytest.mark.parametrize("max_keys", [1, 64, 70])
@pytest.mark.parametrize("hd", [48, 64, 80, 96, 112, 128])
def test_decode_attention_edges(hd, max_keys):
    """B = 64, H = 4; lengths 0, 1, 63, 64, 65, max_keys, max_keys + 9 among the rows; q, the output, the K/V rows and the map
    rows all wider than needed (NaN in what is only skipped, the sentinel kept in what is only left alone)"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(1000 + hd + max_keys)
    B, H, rows, t = 64, 4, 5, 3
    d = H * hd
    ldq, ldo, ldr, mld = d + 8, d + 3, 2 * d + 4, max_keys + 3
    lens = _edge_lens(B, max_keys)
    eff = lens.clamp(max=max_keys)
    mem = torch.randn(B, max_keys, ldr, generator=g)
    mem[:, :, 2 * d:] = NAN
    for b in range(B):
        mem[b, int(eff[b]):] = NAN
    q = torch.randn(B, ldq, generator=g)
    q[:, d:] = NAN
    qd, memd, lens_d = q.cuda(), mem.cuda(), lens.cuda()
    wsb = lib.ttts_decode_attention_workspace_bytes(B, H, hd, max_keys)
    ws = torch.zeros(wsb // 4, device="cuda")
    want = _attn_ref(q[:, :d], mem[:, :, :d], mem[:, :, d:2 * d], eff, H, hd)

    def run(t_, with_map, ended=()):
        st = _rows_state(t_, [4 if b in ended else -1 for b in range(B)])
        out, chk = guarded((B, ldo), SENT)
        amap, chk_m = guarded((B * H, rows, mld), SENT)
        _lib.check(lib.ttts_decode_attention_rows(_p(qd), ldq, _p(memd), _p(memd, d), ldr, max_keys * ldr, _i64(lens_d), _p(out),
                                                  ldo, _p(ws), wsb, B, H, hd, max_keys, _p(st, 8), _p(amap) if with_map else None,
                                                  rows * mld if with_map else 0, mld if with_map else 0, rows if with_map else 0,
                                                  _p(st), s), "ttts_decode_attention_rows")
        torch.cuda.synchronize()
        chk()
        chk_m()
        assert bool((out[:, d:] == SENT).all())
        return out[:, :d].clone(), amap.view(B, H, rows, mld)

    out, amap = run(t, True)
    assert bool(torch.isfinite(out).all())
    e = rel_l2(out, want)
    assert e <= KERNEL_GATE, (hd, max_keys, e)
    got = amap[:, :, t - 1].double().cpu()
    assert bool((torch.cat([amap[:, :, :t - 1], amap[:, :, t:]], dim=2) == SENT).all())
    assert bool((got[:, :, max_keys:] == SENT).all())                   # the columns behind max_keys are left alone
    for b in range(B):
        L = int(eff[b])
        assert bool((got[b, :, L:max_keys] == 0).all()), (hd, max_keys, b, L)
        if L == 0:
            assert bool((out[b] == 0).all()), (hd, max_keys, b)
            continue
        e = rel_l2(got[b, :, :L], _softmax_rows(q[b, :d], mem[b, :, :d], L, H, hd))
        assert e <= KERNEL_GATE, (hd, max_keys, b, L, e)
        assert float((got[b, :, :max_keys].sum(dim=-1) - 1).abs().max()) <= 1e-5, (hd, max_keys, b, L)
    # the kernels without a map, with and without per-row state: the same context, bit for bit
    plain, untouched = run(t, False)
    assert torch.equal(plain, out) and bool((untouched == SENT).all())
    o2, chk2 = guarded((B, ldo), SENT)
    st = S1._state(t)
    _lib.check(lib.ttts_decode_attention(_p(qd), ldq, _p(memd), _p(memd, d), ldr, max_keys * ldr, _i64(lens_d), _p(o2), ldo,
                                         _p(ws), wsb, B, H, hd, max_keys, _p(st), s), "ttts_decode_attention")
    torch.cuda.synchronize()
    chk2()
    assert torch.equal(o2[:, :d], out) and bool((o2[:, d:] == SENT).all())
    # map_rows == t - 1: the context is written, the map is not touched
    late, untouched = run(rows + 1, True)
    assert torch.equal(late, out) and bool((untouched == SENT).all())
    # ended rows on both sides of row 16 keep the sentinel everywhere
    ended = (2, 16, 40, 63)
    o3, m3 = run(t, True, ended)
    for b in range(B):
        if b in ended:
            assert bool((o3[b] == SENT).all()) and bool((m3[b] == SENT).all()), b
        else:
            assert torch.equal(o3[b], out[b]) and torch.equal(m3[b], amap[b]), b


def _attn_ref32(q, k, v, lens, H, hd):
    """_attn_ref's arithmetic in fp32"""
    B = q.shape[0]
    out = torch.zeros(B, H * hd, dtype=torch.float32)
    for b in range(B):
        L = int(lens[b])
        qh = q[b].view(H, hd) / hd ** 0.5
        kh = k[b, :L].view(L, H, hd).transpose(0, 1)
        vh = v[b, :L].view(L, H, hd).transpose(0, 1)
        p = torch.softmax(torch.einsum("hd,hkd->hk", qh, kh), dim=-1)
        out[b] = torch.einsum("hk,hkd->hd", p, vh).reshape(-1)
    return out


def _onehot_inputs(where):
    """B = 8, H = 4, head_dim 64, up to 200 keys; q x 30 (score spread ~30: a handful of keys carry the softmax); per (b, h) the
    key with the largest score swapped into the last position below the length (`where` "last") or into position 0 ("first")"""
    g = torch.Generator().manual_seed(1100)
    B, H, hd, Tk = 8, 4, 64, 200
    d = H * hd
    lens = torch.tensor([200, 200, 200, 200, 193, 192, 130, 65], dtype=torch.int64)
    q = 30.0 * torch.randn(B, d, generator=g)
    k, v = torch.randn(B, Tk, d, generator=g), torch.randn(B, Tk, d, generator=g)
    for b in range(B):
        L = int(lens[b])
        for h in range(H):
            c = slice(h * hd, (h + 1) * hd)
            top = int((k[b, :L, c].double() @ q[b, c].double()).argmax())
            dst = L - 1 if where == "last" else 0
            for a in (k, v):
                tmp = a[b, dst, c].clone()
                a[b, dst, c] = a[b, top, c]
                a[b, top, c] = tmp
    return q, k, v, lens, H, hd


@pytest.mark.parametrize("where", ["last", "first"])
def test_decode_attention_one_hot(where):
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    q, k, v, lens, H, hd = _onehot_inputs(where)
    B, Tk, d = k.shape
    want = _attn_ref(q, k, v, lens, H, hd)
    cpu = rel_l2(_attn_ref32(q, k, v, lens, H, hd), want)
    mem = torch.cat([k, v], dim=2)
    for b in range(B):
        mem[b, int(lens[b]):] = NAN
    qd, memd, lens_d = q.cuda(), mem.cuda(), lens.cuda()
    wsb = lib.ttts_decode_attention_workspace_bytes(B, H, hd, Tk)
    ws = torch.zeros(wsb // 4, device="cuda")
    st = _rows_state(2, [-1] * B)
    out, chk = guarded((B, d), NAN)
    amap, chk_m = guarded((B * H, 3, Tk), SENT)
    _lib.check(lib.ttts_decode_attention_rows(_p(qd), d, _p(memd), _p(memd, d), 2 * d, Tk * 2 * d, _i64(lens_d), _p(out), d, _p(ws),
                                              wsb, B, H, hd, Tk, _p(st, 8), _p(amap), 3 * Tk, Tk, 3, _p(st), s),
               "ttts_decode_attention_rows")
    torch.cuda.synchronize()
    chk()
    chk_m()
    e = rel_l2(out, want)
    print(f"one-hot attention, maximum {where}: fp32 on this CPU {cpu:.3e} (recorded {ONEHOT_CPU[where]:.3e}), the kernel {e:.3e}")
    assert e <= 4 * ONEHOT_CPU[where], (where, e, ONEHOT_CPU[where])
    got = amap.view(B, H, 3, Tk)[:, :, 1].double().cpu()
    for b in range(B):
        L = int(lens[b])
        assert float((got[b].sum(dim=-1) - 1).abs().max()) <= 1e-5, (where, b)
        assert bool((got[b, :, L:] == 0).all()), (where, b)
        peak = got[b].argmax(dim=-1).tolist()
        assert peak == [L - 1 if where == "last" else 0] * H, (where, b, peak)


# ------------------------------------------------------------------------------------------------ A4: frame out, the stop decision
def _frame_out_inputs(B, d, seed, low_row=None):
    """x (B, d), heads, and the fp64 stop logits; with `low_row`, that row's x is moved along the stop weights until its logit
    is 1 below every other row's"""
    g = torch.Generator().manual_seed(seed)
    nm = 80
    x = torch.randn(B, d, generator=g)
    wm, bm = torch.randn(nm, d, generator=g) / d ** 0.5, torch.randn(nm, generator=g)
    wsp, bsp = torch.randn(1, d, generator=g) / d ** 0.5, torch.tensor([0.1])

    def logits():
        return (x.double() @ wsp.double().T).squeeze(1) + bsp.double()

    if low_row is not None:
        lg = logits()
        others = torch.cat([lg[:low_row], lg[low_row + 1:]])
        w = wsp.double()[0]
        x[low_row] = (x[low_row].double() - (lg[low_row] - (others.min() - 1.0)) / (w @ w) * w).float()
    return x, wm, bm, wsp, bsp, logits()


def _frame_out(lib, s, B, d, t, dev, st, row_end=None, cap=8):
    """one ttts_decode_frame_out(_rows) call on sentinel-filled, guarded ys (B, cap, 80) and stop (B, cap)"""
    from transformertts_amd import _lib
    nm = 80
    ys, chk_y = guarded((B, cap, nm), SENT)
    stop, chk_s = guarded((B, cap), SENT)
    args = [_p(t_) for t_ in dev] + [_p(ys), cap * nm, _p(stop), cap, B, d, nm]
    if row_end is None:
        _lib.check(lib.ttts_decode_frame_out(*args, _p(st), s), "ttts_decode_frame_out")
    else:
        _lib.check(lib.ttts_decode_frame_out_rows(*args, row_end, _p(st), s), "ttts_decode_frame_out_rows")
    torch.cuda.synchronize()
    chk_y()
    chk_s()
    rest_y = torch.cat([ys[:, :t], ys[:, t + 1:]], dim=1)
    rest_s = torch.cat([stop[:, :t - 1], stop[:, t:]], dim=1)
    assert bool((rest_y == SENT).all()) and bool((rest_s == SENT).all())
    return ys[:, t].clone(), stop[:, t - 1].clone()


@pytest.mark.parametrize("d", [256, 512, 1024, 2048])
@pytest.mark.parametrize("B", [1, 4, 15, 16, 17, 33, 64, 67])
def test_frame_out_vs_fp64(B, d):
    lib, s = _lib_stream()
    t = 5
    x, wm, bm, wsp, bsp, logits = _frame_out_inputs(B, d, 1200 + B + d)
    dev = [a.cuda() for a in (x, wm, bm, wsp, bsp)]
    st = S1._state(t, thr=2.0)
    mel, stop = _frame_out(lib, s, B, d, t, dev, st)
    e = rel_l2(mel, x.double() @ wm.double().T + bm.double())
    assert e <= KERNEL_GATE, (B, d, e)
    e = rel_l2(stop, logits)
    assert e <= KERNEL_GATE, (B, d, e)
    assert st.cpu()[:3].tolist() == [t + 1, 1 << 40, -1]


@pytest.mark.parametrize("d", [256, 512, 1024, 2048])
@pytest.mark.parametrize("B", [17, 33, 64, 67])
def test_frame_out_stop_decision_past_row_15(B, d):
    """one row held 1 logit below all others, in every pass of the stop kernel's row loop: a threshold between it and the
    others is not a stop frame, one just under it is"""
    lib, s = _lib_stream()
    t = 5
    for hold in sorted({0, 15, 16, 31, 32, B - 1}):
        if hold >= B:
            continue
        x, wm, bm, wsp, bsp, logits = _frame_out_inputs(B, d, 1300 + B + d, low_row=hold)
        p = torch.sigmoid(logits)
        others = torch.cat([p[:hold], p[hold + 1:]])
        assert float(p[hold]) < float(others.min())
        dev = [a.cuda() for a in (x, wm, bm, wsp, bsp)]
        for thr, want in ((0.5 * (float(p[hold]) + float(others.min())), -1), (float(p[hold]) - 2 * MARGIN, t)):
            assert float((p - thr).abs().min()) >= MARGIN, (B, d, hold, thr)
            st = S1._state(t, thr=thr)
            mel, stop = _frame_out(lib, s, B, d, t, dev, st)
            e = rel_l2(stop, logits)
            assert e <= KERNEL_GATE, (B, d, hold, e)
            assert st.cpu()[:3].tolist() == [t + 1, 1 << 40, want], (B, d, hold, thr, st.cpu()[:4].tolist())


@pytest.mark.parametrize("B,d", [(17, 256), (33, 1024), (64, 512), (67, 2048)])
def test_frame_out_rows_latch_past_row_15(B, d):
    lib, s = _lib_stream()
    t = 5
    x, wm, bm, wsp, bsp, logits = _frame_out_inputs(B, d, 1400 + B + d)
    p = torch.sigmoid(logits)
    dev = [a.cuda() for a in (x, wm, bm, wsp, bsp)]
    pad = [1] * (-B % 4)

    def run(row_end, thr, flags=PER_ROW):
        st = _rows_state(t, row_end, thr=thr, flags=flags)
        mel, stop = _frame_out(lib, s, B, d, t, dev, st, row_end=_p(st, 8))
        stc = st.cpu()
        assert stc[4 + B:].tolist() == pad                             # the padding entries are never written
        assert int(stc[0]) == t + 1
        return mel, stop, stc[4:4 + B].tolist(), int(stc[2])

    ref_mel, ref_stop, re, sf = run([-1] * B, 2.0)
    assert re == [-1] * B and sf == -1
    assert rel_l2(ref_stop, logits) <= KERNEL_GATE
    # a mixed state: ended rows on both sides of row 16, about half of the running rows cross
    ended = sorted({1, 16, 18, B - 2})
    start = [7 if b in ended else (-1 if b % 3 else 0) for b in range(B)]
    live = [b for b in range(B) if b not in ended]
    ps = sorted(float(p[b]) for b in live)
    gaps = [(ps[i + 1] - ps[i], i) for i in range(len(ps) // 4, 3 * len(ps) // 4)]
    i = max(gaps)[1]
    thr = 0.5 * (ps[i] + ps[i + 1])
    assert float((p - thr).abs().min()) >= MARGIN, (B, d, float((p - thr).abs().min()))
    crossing = [b for b in live if float(p[b]) >= thr]
    if B >= 33:
        assert any(b >= 16 for b in crossing) and any(b >= 16 for b in live if b not in crossing)
    mel, stop, re, sf = run(start, thr)
    assert re == [start[b] if b in ended else (t if b in crossing else start[b]) for b in range(B)], re
    assert sf == -1
    for b in range(B):
        if b in ended:
            assert bool((mel[b] == SENT).all()) and float(stop[b]) == SENT, b
        else:
            assert torch.equal(mel[b], ref_mel[b]) and torch.equal(stop[b], ref_stop[b]), b
    # the last running rows: row 3 and one row past 15 (in the second pass, and in the last one)
    for last in sorted({16, B - 1}):
        only = [4] * B
        only[3] = only[last] = -1
        lo, hi = sorted((3, last), key=lambda b: float(p[b]))
        mid = 0.5 * (float(p[lo]) + float(p[hi]))
        assert float(p[hi]) - mid >= MARGIN
        mel, stop, re, sf = run(only, mid)                             # one of the two crosses: no stop frame yet
        want = list(only)
        want[hi] = t
        assert re == want and sf == -1, (last, re, sf)
        mel, stop, re, sf = run(only, float(p[lo]) - 2 * MARGIN)      # both cross: this is the stop frame
        want[lo] = t
        assert re == want and sf == t, (last, re, sf)
        alone = [4] * B                                                # the row past 15 alone
        alone[last] = 0
        mel, stop, re, sf = run(alone, float(p[last]) + 2 * MARGIN)
        assert re == alone and sf == -1, (last, re, sf)
        mel, stop, re, sf = run(alone, float(p[last]) - 2 * MARGIN)
        want = list(alone)
        want[last] = t
        assert re == want and sf == t, (last, re, sf)
        assert torch.equal(mel[last], ref_mel[last]) and bool((mel[:last] == SENT).all()) and bool((mel[last + 1:] == SENT).all())
        # without the flag nothing is latched; the decision is over the running rows
        mel, stop, re, sf = run(alone, float(p[last]) - 2 * MARGIN, flags=0)
        assert re == alone and sf == t, (last, re, sf)


# ------------------------------------------------------------------------------------------------ A5: mask_rows
@pytest.mark.parametrize("outer,group,T,C", [(4, 1, 9, 8), (6, 2, 300, 256)])
def test_mask_rows_offset_base_and_clamped_lengths(outer, group, T, C):
    """a base pointer one float past a 16-byte boundary with C % 4 == 0 (the single-float path), lengths below 0 and above T"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    n = outer * T * C
    full, check = guarded((n + 1,), 0.0, guard_rows=64)
    src = torch.randn(n + 1) + 3.0
    full.copy_(src)
    assert full.data_ptr() % 16 == 0
    lens = torch.tensor([-3, T + 5, 4, 0, T, 1][:outer // group], dtype=torch.int64)
    _lib.check(lib.ttts_mask_rows(_p(full, 1), _i64(lens.cuda()), outer, group, T, C, s), "ttts_mask_rows")
    torch.cuda.synchronize()
    check()
    want = src[1:].clone().view(outer, T, C)
    for o in range(outer):
        want[o, max(0, min(T, int(lens[o // group]))):] = 0.0
    assert float(full[0]) == float(src[0])
    assert torch.equal(full[1:].cpu().view(outer, T, C), want)


# ------------------------------------------------------------------------------------------------ B: the engine
def _free_run(cfg_name, w_seed, b_seed, B, Tp, max_len):
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build(cfg_name, w_seed)
    batch, ph, pl = _batch(cfg, B, Tp, b_seed)
    synth = Synthesizer(m)
    out = synth(ph, pl, max_len=max_len, stop_threshold=2.0)
    return cfg, m, synth, batch, ph, pl, out


def _vs_oracle(cfg, w_seed, batch, out, max_len, what):
    from oracle import oracle_inference
    ref = oracle_inference(_oracle64(cfg, w_seed), cfg, batch["phoneme"], batch["phoneme_lens"], max_len=max_len,
                           stop_threshold=2.0)
    for k in KEYS:
        assert out[k].shape == tuple(ref[k].shape), (what, k, out[k].shape, ref[k].shape)
        e = rel_l2(out[k], ref[k])
        assert e < GATE, (what, k, e)


@pytest.mark.parametrize("B,max_len", [(17, 24), (64, 20)])
def test_call_at_shipped_widths_vs_fp64_oracle_and_inference(B, max_len):
    cfg, m, synth, batch, ph, pl, out = _free_run("base", 161 + B, 261 + B, B, 50, max_len)
    assert out["pred_melspec"].shape == (B, max_len - 1, cfg["n_mels"])
    _vs_oracle(cfg, 161 + B, batch, out, max_len, B)
    fast = m.inference(ph, pl, max_len=max_len, stop_threshold=2.0, use_kv_cache=True)
    for k in KEYS:
        assert out[k].shape == fast[k].shape, k
        e = rel_l2(out[k], fast[k])
        assert e < 1e-5, (B, k, e)


def test_scaled_b9_vs_fp64_oracle():
    """the scaled model at B >= 8: d_ffn 2048 on the two-columns-per-wave GEMV (decode_linear_kernel<8,2>)"""
    cfg, m, synth, batch, ph, pl, out = _free_run("scaled", 171, 172, 9, 40, 12)
    assert cfg["decoder_d_ffn"] == 2048
    _vs_oracle(cfg, 171, batch, out, 12, "scaled")


def test_rows_of_a_64_batch_do_not_depend_on_it():
    cfg, m, synth, batch, ph, pl, full = _free_run("base", 181, 182, 64, 50, 33)
    for i in (0, 16, 40, 63):
        alone = synth(ph[i:i + 1], pl[i:i + 1], max_len=33, stop_threshold=2.0)
        for k in KEYS:
            e = rel_l2(alone[k], full[k][i:i + 1])
            assert alone[k].shape[1] == 32 and e < 1e-5, (i, k, e)


# B * F = 80 = n_mels rows: the fit of the stop head is still exact.  Frames per graph: 2.  Row 16 ends first (frame 1, alone),
# row 19 last (frame 4 = max_len - 1, by crossing, alone: it ends the call), rows 17 and 19 end on chunk boundaries
B20_CROSSINGS = [2, 3] * 8 + [1, 2, 3, 4]


def test_synthesize_b20_prescribed_ends():
    from oracle import oracle_inference
    from transformertts_amd.synthesis import Synthesizer
    B, max_len, chunk, thr = 20, 5, 2, 0.5
    F = max_len - 1
    cfg, m = _build("base", 191)
    batch, ph, pl = _batch(cfg, B, 50, 192)
    synth = Synthesizer(m, chunk=chunk)
    probe = synth(ph, pl, max_len=max_len, stop_threshold=2.0)
    assert B * F <= cfg["n_mels"]
    res = _fit_stop_head(m, probe["pred_melspec"], _ramps(B20_CROSSINGS, F))
    free = synth(ph, pl, max_len=max_len, stop_threshold=2.0)          # the same frames, the refitted stop logits
    assert torch.equal(free["pred_melspec"], probe["pred_melspec"])
    sd = _oracle64(cfg, 191, m)
    ref = oracle_inference(sd, cfg, batch["phoneme"], batch["phoneme_lens"], max_len=max_len, stop_threshold=2.0)
    p64 = torch.sigmoid(ref["pred_stop"][..., 0])
    want, margin = _first_crossings(p64, thr, max_len)
    p32 = torch.sigmoid(free["pred_stop"][..., 0].double()).cpu()
    margin = min(margin, float((p32 - thr).abs().min()))
    print(f"B = 20: fit residual {res:.1e}, fp64 ends {want.tolist()}, margin {margin:.4f}")
    assert margin >= MARGIN, margin
    want = want.tolist()
    assert want == B20_CROSSINGS, want
    assert min(want) == want[16] and want.count(min(want)) == 1 and max(want) == want[19] and want.count(max(want)) == 1
    assert want[17] % chunk == 0
    out = synth.synthesize(ph, pl, max_len=max_len, stop_threshold=thr, alignments=True)
    assert out["mel_lens"].tolist() == want, (out["mel_lens"].tolist(), want)
    T = max(want)
    assert out["pred_melspec"].shape == (B, T, cfg["n_mels"]) and out["pred_stop"].shape == (B, T, 1)
    _assert_zero_behind(out, out["mel_lens"])
    plain = synth.synthesize(ph, pl, max_len=max_len, stop_threshold=thr)
    for k in KEYS + ("mel_lens",):
        assert torch.equal(plain[k], out[k]), k
    for b, n in enumerate(want):
        assert torch.equal(out["pred_melspec"][b, :n], free["pred_melspec"][b, :n]), b
        assert torch.equal(out["pred_stop"][b, :n], free["pred_stop"][b, :n]), b
        for k in ("pred_melspec", "pred_stop"):                        # (the post-net of a row's own frames: rows 16, 19 below)
            e = rel_l2(out[k][b, :n], ref[k][b, :n])
            assert e < GATE, (b, k, e)
    sel = [0, 16, 19]
    maps = _oracle_alignments(sd, cfg, batch["phoneme"][sel], batch["phoneme_lens"][sel], out["pred_melspec"][sel].double().cpu())
    assert len(maps) == len(out["alignments"]) == cfg["decoder_n_layers"]
    for i, (a, r) in enumerate(zip(out["alignments"], maps)):
        assert a.shape == (B, cfg["decoder_n_head"], T, ph.shape[1]), (i, a.shape)
        for j, b in enumerate(sel):
            n = want[b]
            e = rel_l2(a[b, :, :n], r[j, :, :n])
            assert e < GATE, (i, b, e)
            assert float((a[b, :, :n].double().sum(-1) - 1).abs().max()) <= 1e-5, (i, b)
    for b in (16, 19):
        n = want[b]
        alone = synth(ph[b:b + 1], pl[b:b + 1], max_len=max_len, stop_threshold=thr)
        assert alone["post_melspec"].shape[1] == n, (b, n, alone["post_melspec"].shape)
        for k in KEYS:
            e = rel_l2(out[k][b, :n], alone[k][0])
            assert e < PATH_GATE, (b, k, e)
        one = oracle_inference(sd, cfg, batch["phoneme"][b:b + 1], batch["phoneme_lens"][b:b + 1], max_len=max_len,
                               stop_threshold=thr)
        assert one["post_melspec"].shape[1] == n
        e = rel_l2(out["post_melspec"][b, :n], one["post_melspec"][0])
        assert e < GATE, (b, e)


@pytest.mark.parametrize("max_len", [256, 257])
def test_decoding_to_the_last_row_of_a_capacity(max_len):
    """max_len = 256 fills a 256-frame capacity to its last row; 257 is the first that needs the next one"""
    from oracle import oracle_forward
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 201)
    batch, ph, pl = _batch(cfg, 2, 40, 202, ragged=False)
    synth = Synthesizer(m)
    out = synth(ph, pl, max_len=max_len, stop_threshold=2.0)
    n = max_len - 1
    assert [k[2] for k in synth.shape_bytes()] == [256 if max_len == 256 else 512]
    pred, stop = out["pred_melspec"], out["pred_stop"][..., 0]
    assert pred.shape == (2, n, cfg["n_mels"]) and stop.shape == (2, n)
    fast = m.inference(ph, pl, max_len=max_len, stop_threshold=2.0, use_kv_cache=True)
    for k in KEYS:
        assert out[k].shape == fast[k].shape, k
        e = rel_l2(out[k], fast[k])
        assert e < 1e-5, (max_len, k, e)
    ml = torch.full((2,), n, dtype=torch.int64)
    m.eval()
    with torch.no_grad():
        fw = m(ph, pred, pl, ml.cuda(), need_alignments=False)
    e = rel_l2(fw["pred_melspec"], pred)
    assert e < 1e-5, e
    e = rel_l2(fw["pred_stop"], stop)
    assert e < 1e-5, e
    ref = oracle_forward(_oracle64(cfg, 201), cfg, batch["phoneme"], pred.double().cpu(), batch["phoneme_lens"], ml,
                         training=False, dropout=False)
    e = rel_l2(pred, ref["pred_melspec"])
    assert e < GATE, e
    e = rel_l2(stop, ref["pred_stop"])
    assert e < GATE, e


@pytest.mark.parametrize("Tp", [64, 65])
def test_phoneme_counts_on_both_sides_of_a_key_block(Tp):
    """Tp = 64 is one key block of the memory exactly, 65 pads to 128 (a second block, empty but for one key); the lengths
    hold Tp and 1"""
    from oracle import oracle_inference
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 211)
    batch, ph, pl = _batch(cfg, 3, Tp, 212, ragged=False)
    lens = torch.tensor([Tp, 30, 1], dtype=torch.int64)
    phon = batch["phoneme"] * (torch.arange(Tp).unsqueeze(0) < lens.unsqueeze(1))
    synth = Synthesizer(m)
    out = synth(phon.cuda(), lens.cuda(), max_len=24, stop_threshold=2.0)
    assert [k[1] for k in synth.shape_bytes()] == [64 if Tp == 64 else 128]
    ref = oracle_inference(_oracle64(cfg, 211), cfg, phon, lens, max_len=24, stop_threshold=2.0)
    fast = m.inference(phon.cuda(), lens.cuda(), max_len=24, stop_threshold=2.0, use_kv_cache=True)
    for k in KEYS:
        assert out[k].shape == tuple(ref[k].shape) == fast[k].shape, k
        e = rel_l2(out[k], ref[k])
        assert e < GATE, (Tp, k, e)
        e = rel_l2(out[k], fast[k])
        assert e < 1e-5, (Tp, k, e)
    al = synth.synthesize(phon.cuda(), lens.cuda(), max_len=24, stop_threshold=2.0, alignments=True)
    for a in al["alignments"]:
        assert a.shape[-1] == Tp
        for b in range(3):
            assert bool((a[b, :, :, int(lens[b]):] == 0).all()), b
            assert float((a[b].double().sum(-1) - 1).abs().max()) <= 1e-5, b
        assert bool((a[2, :, :, 0] == 1).all())                        # one key: all of the weight


@pytest.mark.parametrize("B", [2, 9])
def test_wide_config_vs_fp64_oracle(B):
    """d_model 1024, d_ffn 4096, head_dim 128: the limits Synthesizer advertises (decode_linear_kernel<4,*> and <16,1>,
    decode_layernorm at 16 values per lane, decode_attn_*<128>)"""
    cfg, m, synth, batch, ph, pl, out = _free_run("wide", 221, 222 + B, B, 30, 10)
    assert cfg["d_model"] == 1024 and cfg["decoder_d_ffn"] == 4096 and cfg["d_model"] // cfg["decoder_n_head"] == 128
    _vs_oracle(cfg, 221, batch, out, 10, ("wide", B))
