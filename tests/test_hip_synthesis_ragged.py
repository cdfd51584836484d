"""Batched synthesis with per-utterance ends (`Synthesizer.synthesize`) and the per-row decode kernels behind it
(csrc/decode.hip, the ttts_decode_*_rows entry points and ttts_mask_rows): one frame with a mixed per-row state through the C
ABI, alignment rows against an fp64 softmax, prescribed stop frames against the free-running call, the per-row B = 1 calls and
the fp64 oracle, alignment maps against an fp64 teacher-forced pass and the training forward, and state hygiene across calls."""
from ctypes import c_void_p

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
GATE = 1e-4          # the engine against the fp64 oracle, as test_hip_model.py / test_hip_synthesis.py
KERNEL_GATE = 1e-6   # one decode kernel against fp64
PATH_GATE = 1e-5     # two fp32 paths of this library
MARGIN = 1e-3        # smallest distance of a stop probability from the threshold a test may rely on
PER_ROW = 1          # TTTS_DECODE_PER_ROW
SENT = 7.0           # what the output buffers hold before a kernel-level call
KEYS = ("pred_melspec", "post_melspec", "pred_stop")


def _p(t, off=0):
    return c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def _state(t, row_end, t_end=1 << 40, thr=0.5, stop=-1, flags=PER_ROW):
    """ttts_decode_state followed by row_end (padded to a multiple of 4 entries with ended rows that do not exist, as the
    kernels may read but never act on them), as one device tensor"""
    pad = [1] * (-len(row_end) % 4)
    st = torch.tensor([t, t_end, stop, 0] + list(row_end) + pad, dtype=torch.int64)
    st.view(torch.float32)[6] = thr
    st.view(torch.int32)[7] = flags
    return st.cuda()


def _lib_stream():
    from transformertts_amd import _lib, ops
    return _lib.load(), ops._stream()


def _no_dropout(m):
    from transformertts_amd.model.layers import MultiheadAttention
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, MultiheadAttention):
            mod.dropout = 0.0


def _build(cfg_name, w_seed):
    from oracle import model_config, fill_state
    from transformertts_amd.model import TransformerTTS
    cfg = model_config(cfg_name)
    m = TransformerTTS(**cfg, device="cuda")
    m.load_state_dict(fill_state(cfg, w_seed), strict=True)
    m = m.to("cuda")
    _no_dropout(m)
    return cfg, m


def _oracle64(cfg, w_seed, m=None):
    """the fp64 state dict of the seed; with `m`, its stop head replaced by the model's (refitted) one"""
    from oracle import fill_state
    sd = fill_state(cfg, w_seed)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    if m is not None:
        sd["linear2.linear.weight"] = m.linear2.linear.weight.detach().double().cpu()
        sd["linear2.linear.bias"] = m.linear2.linear.bias.detach().double().cpu()
    return sd


def _batch(cfg, B, Tp, seed, ragged=True):
    from oracle import synth_batch
    b = synth_batch(B, Tp, 40, cfg["n_mels"], cfg["n_phon"], ragged=ragged, seed=seed)
    return b, b["phoneme"].cuda(), b["phoneme_lens"].cuda()


def _fit_stop_head(m, mel, target):
    """make the stop logit of frame f of row b of `mel` (B, F, n_mels) follow target[b, f]: the stop head becomes a combination
    of the mel head's rows (it does not feed back into the frames, so the frames stay what they were).  Exact when
    B * F <= n_mels.  Returns the fp64 residual of the fit."""
    wm, bm = m.linear1.linear.weight.detach().double().cpu(), m.linear1.linear.bias.detach().double().cpu()
    A = (mel.double().cpu() - bm).reshape(-1, wm.shape[0])
    y = target.double().reshape(-1)
    a = torch.linalg.pinv(A) @ y
    m.linear2.linear.weight.data.copy_((a @ wm).float().view(1, -1))
    m.linear2.linear.bias.data.zero_()
    return float((A @ a - y).abs().max())


def _ramps(crossings, F):
    """(B, F) stop logits 0.5 * (f - c + 0.5) over the 1-based frames f: row b first reaches 0 (probability 0.5) at f = c_b"""
    f = torch.arange(1, F + 1, dtype=torch.float64)
    return torch.stack([0.5 * (f - c + 0.5) for c in crossings])


def _first_crossings(p, thr, max_len):
    """per-row end frames from (B, F) stop probabilities, and the smallest distance of any of them from the threshold"""
    hit = p >= thr
    F = p.shape[1]
    first = torch.where(hit.any(dim=1), hit.double().argmax(dim=1) + 1, torch.full((p.shape[0],), max_len - 1))
    assert F == max_len - 1
    return first.to(torch.int64), float((p - thr).abs().min())


def _assert_zero_behind(out, lens):
    for b, n in enumerate(lens.tolist()):
        for k in KEYS:
            assert bool((out[k][b, n:] == 0).all()), (k, b, n)
        for a in out.get("alignments", []):
            assert bool((a[b, :, n:] == 0).all()), (b, n)


# ------------------------------------------------------------------------------------------------ kernels through the C ABI
def _one_frame(row_end, thr, flags=PER_ROW, seed=5):
    """one decoder-shaped frame (frame in, in-projection into the cache, self-attention, out-projection + residual, LayerNorm,
    cross-attention with its map row, frame out) on sentinel-filled outputs; returns every buffer and the state read back"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(seed)
    B, d, H, nm, cap, t, Tk = len(row_end), 256, 4, 80, 40, 13, 128
    hd = d // H

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda()

    ys = rnd(B, cap, nm)
    ys[:, t:] = SENT
    w1, b1, w2, b2 = rnd(d, nm, scale=nm ** -0.5), rnd(d), rnd(d, d, scale=d ** -0.5), rnd(d)
    pe, alpha = rnd(100, d), torch.tensor([0.7]).cuda()
    w_in, b_in = rnd(3 * d, d, scale=d ** -0.5), rnd(3 * d)
    w_o, b_o = rnd(d, d, scale=d ** -0.5), rnd(d)
    gam, bet = rnd(d), rnd(d)
    wm, bm, wsp, bsp = rnd(nm, d, scale=d ** -0.5), rnd(nm), rnd(1, d, scale=d ** -0.5), torch.tensor([0.1]).cuda()
    cache = rnd(B, cap, 2 * d)
    cache[:, t - 1:] = SENT
    mem = rnd(B, Tk, 2 * d)
    lens = torch.tensor([(37 * (b + 1)) % Tk + 1 for b in range(B)], dtype=torch.int64).cuda()
    buf = {k: torch.full((B, d), SENT, device="cuda") for k in ("tmp", "h", "q", "ctx", "res", "h2", "ctx2")}
    stop = torch.full((B, cap), SENT, device="cuda")
    amap = torch.full((B, H, cap, Tk), SENT, device="cuda")
    wsb = max(lib.ttts_decode_attention_workspace_bytes(B, H, hd, cap), lib.ttts_decode_attention_workspace_bytes(B, H, hd, Tk))
    ws = torch.zeros(wsb // 4, device="cuda")
    st = _state(t, row_end, thr=thr, flags=flags)
    re = _p(st, 8)
    ck = _lib.check
    ck(lib.ttts_decode_frame_in_rows(_p(ys), cap * nm, nm, _p(w1), _p(b1), _p(w2), _p(b2), _p(pe), _p(alpha), _p(buf["tmp"]),
                                     _p(buf["h"]), B, d, re, _p(st), s), "frame_in_rows")
    ck(lib.ttts_decode_linear_rows(_p(buf["h"]), d, 0, _p(w_in), _p(b_in), None, 0, _p(buf["q"]), d, 0, _p(cache), cap * 2 * d,
                                   2 * d, d, B, 3 * d, d, 0, re, _p(st), s), "linear_rows")
    ck(lib.ttts_decode_attention_rows(_p(buf["q"]), d, _p(cache), _p(cache, d), 2 * d, cap * 2 * d, None, _p(buf["ctx"]), d,
                                      _p(ws), wsb, B, H, hd, cap, re, None, 0, 0, 0, _p(st), s), "attention_rows")
    ck(lib.ttts_decode_linear_rows(_p(buf["ctx"]), d, 0, _p(w_o), _p(b_o), _p(buf["h"]), d, _p(buf["res"]), d, 0, None, 0, 0, d, B,
                                   d, d, 0, re, _p(st), s), "linear_rows")
    ck(lib.ttts_decode_layernorm_rows(_p(buf["res"]), _p(gam), _p(bet), _p(buf["h2"]), B, d, 1e-5, re, _p(st), s),
       "layernorm_rows")
    ck(lib.ttts_decode_attention_rows(_p(buf["h2"]), d, _p(mem), _p(mem, d), 2 * d, Tk * 2 * d, _p(lens), _p(buf["ctx2"]), d,
                                      _p(ws), wsb, B, H, hd, Tk, re, _p(amap), cap * Tk, Tk, cap, _p(st), s), "attention_rows")
    ck(lib.ttts_decode_frame_out_rows(_p(buf["ctx2"]), _p(wm), _p(bm), _p(wsp), _p(bsp), _p(ys), cap * nm, _p(stop), cap, B, d, nm,
                                      re, _p(st), s), "frame_out_rows")
    torch.cuda.synchronize()
    out = dict(buf)
    out.update(cache_row=cache[:, t - 1].clone(), cache_rest=cache[:, t:].clone(), ys_row=ys[:, t].clone(),
               ys_rest=ys[:, t + 1:].clone(), stop_row=stop[:, t - 1].clone(), map_row=amap[:, :, t - 1].clone(),
               map_rest=torch.cat([amap[:, :, :t - 1], amap[:, :, t:]], dim=2), lens=lens.cpu())
    stc = st.cpu()
    assert stc[4 + B:].tolist() == [1] * (-B % 4)                  # the padding entries are never written
    return out, stc[:4 + B], t


# 6 rows: one column per wave in the GEMV, a workgroup with one ended row and a clamped one; 11 rows: four columns per wave,
# workgroups with one, three and two ended rows
@pytest.mark.parametrize("mixed", [[-1, 5, -1, 0, 9, -1], [-1, 5, -1, 0, 9, -1, 3, 3, 12, 1, 0]])
def test_one_frame_with_a_mixed_row_state(mixed):
    """ended rows keep the sentinel in every output, running rows get bit for bit what they get with no row ended; the latch
    records a row's first crossing only and the stop frame appears exactly when no row is left running"""
    B = len(mixed)                            # row_end > 0: ended at that frame; 0 and -1 both mean "running"
    ended = [b for b in range(B) if mixed[b] > 0]
    live = [b for b in range(B) if mixed[b] <= 0]
    ref, st_ref, t = _one_frame([-1] * B, thr=2.0)
    assert st_ref[4:].tolist() == [-1] * B and int(st_ref[2]) == -1 and int(st_ref[0]) == t + 1
    p = 1.0 / (1.0 + torch.exp(-ref["stop_row"].double().cpu()))
    order = sorted(live, key=lambda b: float(p[b]))
    thr = 0.5 * (float(p[order[1]]) + float(p[order[2]]))          # the two lowest running rows stay below it
    assert float((p - thr).abs().min()) >= MARGIN
    crossing = [b for b in live if float(p[b]) >= thr]
    assert len(crossing) == len(live) - 2
    out, st, _ = _one_frame(mixed, thr=thr)
    names = ("tmp", "h", "q", "ctx", "res", "h2", "ctx2", "cache_row", "ys_row", "stop_row", "map_row")
    for k in names:
        for b in ended:
            assert bool((out[k][b] == SENT).all()), (k, b)
        for b in live:
            assert torch.equal(out[k][b], ref[k][b]) and not bool((out[k][b] == SENT).all()), (k, b)
    for k in ("cache_rest", "ys_rest", "map_rest"):
        assert bool((out[k] == SENT).all()) and bool((ref[k] == SENT).all()), k
    want = [mixed[b] if b in ended else (t if b in crossing else mixed[b]) for b in range(B)]
    assert st[4:].tolist() == want, (st[4:].tolist(), want)
    assert int(st[2]) == -1 and int(st[0]) == t + 1               # two rows are still running
    # every running row crosses: each gets t, the ended ones keep their first crossing, and this is the stop frame
    out, st, _ = _one_frame(mixed, thr=0.0)
    assert st[4:].tolist() == [mixed[b] if b in ended else t for b in range(B)]
    assert int(st[2]) == t and int(st[0]) == t + 1
    for b in ended:
        assert bool((out["stop_row"][b] == SENT).all())
    # without the flag row_end is only read: the decision is the all-rows one over the running rows, nothing is latched
    out, st, _ = _one_frame(mixed, thr=0.0, flags=0)
    assert st[4:].tolist() == mixed and int(st[2]) == t
    out, st, _ = _one_frame(mixed, thr=thr, flags=0)
    assert st[4:].tolist() == mixed and int(st[2]) == -1
    for b in live:
        assert torch.equal(out["ys_row"][b], ref["ys_row"][b])
    # a decode that is over (stop recorded) leaves everything alone, row state included
    lib, s = _lib_stream()
    done = _state(t, mixed, stop=3)
    y = torch.full((B, 256), SENT, device="cuda")
    x = torch.randn(B, 256, device="cuda")
    gam = torch.ones(256, device="cuda")
    assert lib.ttts_decode_layernorm_rows(_p(x), _p(gam), _p(gam), _p(y), B, 256, 1e-5, _p(done, 8), _p(done), s) == 0
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and done.cpu()[4:4 + B].tolist() == mixed


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_map_rows_vs_fp64_softmax(hd):
    """the alignment row of a frame: softmax(q k^T / sqrt(hd)) over the keys below the length, exact zeros from there to
    max_keys, for key counts on both sides of a 64-key block boundary; the context vector is what the map-less kernels give"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(300 + hd)
    H = 256 // hd if hd < 128 else 2
    d = H * hd
    lens = torch.tensor([1, 63, 64, 65, 127, 128, 129, 200], dtype=torch.int64)
    B, Tk, rows, t = lens.numel(), 200, 6, 4
    mem = torch.randn(B, Tk, 2 * d, generator=g)
    for b in range(B):
        mem[b, int(lens[b]):] = float("nan")                      # never read
    q = torch.randn(B, d, generator=g).cuda()
    memd, lens_d = mem.cuda(), lens.cuda()
    wsb = lib.ttts_decode_attention_workspace_bytes(B, H, hd, Tk)
    ws = torch.zeros(wsb // 4, device="cuda")
    st = _state(t, [-1] * B)
    amap = torch.full((B, H, rows, Tk), SENT, device="cuda")
    out = torch.full((B, d), SENT, device="cuda")
    _lib.check(lib.ttts_decode_attention_rows(_p(q), d, _p(memd), _p(memd, d), 2 * d, Tk * 2 * d, _p(lens_d), _p(out), d, _p(ws),
                                              wsb, B, H, hd, Tk, _p(st, 8), _p(amap), rows * Tk, Tk, rows, _p(st), s),
               "ttts_decode_attention_rows")
    plain = torch.full((B, d), SENT, device="cuda")
    _lib.check(lib.ttts_decode_attention(_p(q), d, _p(memd), _p(memd, d), 2 * d, Tk * 2 * d, _p(lens_d), _p(plain), d, _p(ws),
                                         wsb, B, H, hd, Tk, _p(st), s), "ttts_decode_attention")
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
    got = amap[:, :, t - 1].double().cpu()                           # (B, H, Tk)
    assert bool((torch.cat([amap[:, :, :t - 1], amap[:, :, t:]], dim=2) == SENT).all())
    for b in range(B):
        L = int(lens[b])
        qh = q[b].double().cpu().view(H, hd) / hd ** 0.5
        kh = mem[b, :L, :d].double().view(L, H, hd).transpose(0, 1)
        want = torch.softmax(torch.einsum("hd,hkd->hk", qh, kh), dim=-1)
        assert rel_l2(got[b, :, :L], want) <= KERNEL_GATE, (hd, L, rel_l2(got[b, :, :L], want))
        assert bool((got[b, :, L:] == 0).all()), (hd, L)
        assert float((got[b].sum(dim=-1) - 1).abs().max()) <= 1e-6, (hd, L, got[b].sum(dim=-1))
    # a frame the planes do not hold (t - 1 >= map_rows) writes no map row
    st = _state(rows + 1, [-1] * B)
    before = amap.clone()
    _lib.check(lib.ttts_decode_attention_rows(_p(q), d, _p(memd), _p(memd, d), 2 * d, Tk * 2 * d, _p(lens_d), _p(out), d, _p(ws),
                                              wsb, B, H, hd, Tk, _p(st, 8), _p(amap), rows * Tk, Tk, rows, _p(st), s),
               "ttts_decode_attention_rows")
    torch.cuda.synchronize()
    assert torch.equal(amap, before) and torch.equal(out, plain)


@pytest.mark.parametrize("outer,group,T,C", [(3, 1, 17, 80), (3, 1, 9, 1), (8, 4, 11, 37), (2, 1, 700, 256), (5, 1, 6, 6)])
def test_mask_rows(outer, group, T, C):
    from conftest import guarded
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    n_len = outer // group
    lens = torch.tensor([(5 * i + 3) % (T + 1) for i in range(n_len)], dtype=torch.int64)
    lens[0] = T                                                      # nothing to zero
    if n_len > 1:
        lens[1] = 0                                                  # everything
    x, check = guarded((outer, T, C), 0.0)
    src = torch.randn(outer, T, C) + 3.0
    x.copy_(src)
    _lib.check(lib.ttts_mask_rows(_p(x), c_void_p(lens.cuda().data_ptr()), outer, group, T, C, s), "ttts_mask_rows")
    torch.cuda.synchronize()
    check()
    want = src.clone()
    for o in range(outer):
        want[o, int(lens[o // group]):] = 0.0
    assert torch.equal(x.cpu(), want)


# ------------------------------------------------------------------------------------------------ the engine
def _prescribed_case(crossings, max_len, chunk):
    """base config, weights seed 81, batch seed 82, B = 4: the stop head refitted so that row b first reaches probability 0.5 at
    frame crossings[b] (None: never).  -> cfg, model, synthesizer, inputs, the free-running reference call, expected lengths"""
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 81)
    batch, ph, pl = _batch(cfg, len(crossings), 60, 82)
    synth = Synthesizer(m, chunk=chunk)
    F = max_len - 1
    probe = synth(ph, pl, max_len=max_len, stop_threshold=2.0)
    assert len(crossings) * F <= cfg["n_mels"]                       # an exact fit
    res = _fit_stop_head(m, probe["pred_melspec"], _ramps([c if c is not None else F + 6 for c in crossings], F))
    assert res <= 1e-9, res
    free = synth(ph, pl, max_len=max_len, stop_threshold=2.0)        # same frames, the refitted stop logits
    assert torch.equal(free["pred_melspec"], probe["pred_melspec"])
    p = torch.sigmoid(free["pred_stop"][..., 0].double()).cpu()
    lens, margin = _first_crossings(p, 0.5, max_len)
    print(f"prescribed {crossings}: fit residual {res:.1e}, engine lengths {lens.tolist()}, margin {margin:.4f}")
    assert margin >= MARGIN, margin
    want = [c if c is not None else F for c in crossings]
    assert lens.tolist() == want, (lens.tolist(), want)
    return cfg, m, synth, batch, ph, pl, free, want


# chunk 9: ends inside the first chunk (5), on a chunk boundary (9), in the second chunk (14), at max_len - 1 by crossing (19);
# chunk 16 (the default): inside the first chunk, on its boundary, in the second chunk, and at max_len - 1 by never crossing
@pytest.mark.parametrize("crossings,chunk", [((5, 9, 14, 19), 9), ((5, 16, 18, None), 16), ((19, None, 5, 5), 16)])
def test_prescribed_stop_frames(crossings, chunk):
    from oracle import oracle_inference
    max_len, thr = 20, 0.5
    cfg, m, synth, batch, ph, pl, free, want = _prescribed_case(crossings, max_len, chunk)
    assert synth.chunk == chunk
    out = synth.synthesize(ph, pl, max_len=max_len, stop_threshold=thr)
    T = max(want)
    assert out["mel_lens"].dtype == torch.int64 and out["mel_lens"].device == ph.device
    assert out["mel_lens"].tolist() == want, (out["mel_lens"].tolist(), want)
    assert out["pred_melspec"].shape == (4, T, cfg["n_mels"]) == out["post_melspec"].shape and out["pred_stop"].shape == (4, T, 1)
    for k in KEYS:
        assert out[k].dtype == free[k].dtype and out[k].device == free[k].device, k
    _assert_zero_behind(out, out["mel_lens"])
    assert synth.captures == 2                   # one chunk graph for __call__, one for synthesize
    sd = _oracle64(cfg, 81, m)
    for b, n in enumerate(want):
        # a row's frames before its end: the free-running call's, bit for bit
        assert torch.equal(out["pred_melspec"][b, :n], free["pred_melspec"][b, :n]), b
        assert torch.equal(out["pred_stop"][b, :n], free["pred_stop"][b, :n]), b
        # the post-net of its own frames: the call on that row alone, which stops at the same frame
        alone = synth(ph[b:b + 1], pl[b:b + 1], max_len=max_len, stop_threshold=thr)
        assert alone["post_melspec"].shape[1] == n, (b, n, alone["post_melspec"].shape)
        e = rel_l2(out["post_melspec"][b, :n], alone["post_melspec"][0])
        assert e < PATH_GATE, (b, e)
        # the fp64 oracle on that row alone (its B = 1 all-stop is the per-row stop)
        ref = oracle_inference(sd, cfg, batch["phoneme"][b:b + 1], batch["phoneme_lens"][b:b + 1], max_len=max_len,
                               stop_threshold=thr)
        assert ref["pred_melspec"].shape[1] == n, (b, n, ref["pred_melspec"].shape)
        for k in KEYS:
            assert out[k][b, :n].shape == tuple(ref[k][0].shape), (k, out[k][b, :n].shape, ref[k][0].shape)
            e = rel_l2(out[k][b, :n], ref[k][0])
            assert e < GATE, (b, k, e)


def test_a_threshold_nobody_reaches_is_the_free_running_call():
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 121)
    _, ph, pl = _batch(cfg, 5, 70, 122)
    synth = Synthesizer(m)
    L = 2 * synth.chunk + 3
    free = synth(ph, pl, max_len=L, stop_threshold=2.0)
    out = synth.synthesize(ph, pl, max_len=L, stop_threshold=2.0)
    assert out["mel_lens"].tolist() == [L - 1] * 5
    for k in KEYS:
        assert torch.equal(out[k], free[k]), k
    assert synth.captures == 2                   # __call__'s graph and synthesize's
    # threshold 0: every row ends at its first frame
    one = synth.synthesize(ph, pl, max_len=L, stop_threshold=0.0)
    assert one["mel_lens"].tolist() == [1] * 5 and one["pred_melspec"].shape[1] == 1
    assert torch.equal(one["pred_melspec"], free["pred_melspec"][:, :1])


def _oracle_alignments(sd, cfg, phoneme, phoneme_lens, pred):
    """fp64 teacher-forced decoder pass over the frames `pred` (B, T, n_mels) on the unmasked-encoder memory, from the oracle's
    own blocks as oracle_inference puts them together: the per-layer (B, H, T, Tp) cross-attention maps"""
    import torch.nn.functional as F
    from oracle.ref_model import conv_norm_bn, decoder_layer, encoder_layer, positional_encoding
    B, T = pred.shape[:2]
    x = F.embedding(phoneme, sd["emb.weight"])
    for i in range(cfg["encoder_prenet_n_layers"]):
        x = conv_norm_bn(sd, f"enc_prenet.layers.{2 * i}", x, False, False)
    x = F.linear(x, sd["enc_prenet.linear.linear.weight"], sd["enc_prenet.linear.linear.bias"])
    x = positional_encoding(sd, x, 0.1, False)
    full = torch.full((B,), phoneme.size(1), dtype=torch.long)
    for i in range(cfg["encoder_n_layers"]):
        x = encoder_layer(sd, f"encoder.layers.{i}", x, cfg["encoder_n_head"], full, cfg["encoder_dropout"], False)
    y = torch.cat([torch.zeros_like(pred[:, :1]), pred[:, :-1]], dim=1)
    y = F.relu(F.linear(y, sd["dec_prenet.linear1.linear.weight"], sd["dec_prenet.linear1.linear.bias"]))
    y = F.relu(F.linear(y, sd["dec_prenet.linear2.linear.weight"], sd["dec_prenet.linear2.linear.bias"]))
    y = positional_encoding(sd, y, 0.1, False)
    lens_t = torch.full((B,), T, dtype=torch.long)
    maps = []
    for i in range(cfg["decoder_n_layers"]):
        y, A = decoder_layer(sd, f"decoder.layers.{i}", y, x, cfg["decoder_n_head"], lens_t, phoneme_lens,
                             cfg["decoder_dropout"], False)
        maps.append(A)
    return maps


def _ragged_case(cfg_name, w_seed, b_seed, B, Tp, max_len, ragged_ph):
    """a model whose stop head is refitted (least squares; exact when B * F <= n_mels) towards ends spread over the frames; the
    expected lengths come from the engine's own free-running stop probabilities, with the margin asserted"""
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build(cfg_name, w_seed)
    batch, ph, pl = _batch(cfg, B, Tp, b_seed, ragged=ragged_ph)
    synth = Synthesizer(m)
    F = max_len - 1
    probe = synth(ph, pl, max_len=max_len, stop_threshold=2.0)
    cross = [max(2, round(F * (b + 1) / (B + 0.5))) for b in range(B)]
    _fit_stop_head(m, probe["pred_melspec"], _ramps(cross, F))
    free = synth(ph, pl, max_len=max_len, stop_threshold=2.0)
    p = torch.sigmoid(free["pred_stop"][..., 0].double()).cpu()
    lens, margin = _first_crossings(p, 0.5, max_len)
    print(f"{cfg_name}: target ends {cross}, engine ends {lens.tolist()}, margin {margin:.4f}")
    assert margin >= MARGIN, margin
    assert len(set(lens.tolist())) > 1                               # the rows do end at different frames
    return cfg, m, synth, batch, ph, pl, free, lens


@pytest.mark.parametrize("cfg_name,w_seed,b_seed,B,Tp,max_len", [("base", 131, 132, 3, 70, 24), ("tiny1h", 133, 134, 2, 12, 9),
                                                                 ("micro", 135, 136, 2, 12, 9)])
def test_alignments_vs_fp64_teacher_forced_pass(cfg_name, w_seed, b_seed, B, Tp, max_len):
    cfg, m, synth, batch, ph, pl, free, lens = _ragged_case(cfg_name, w_seed, b_seed, B, Tp, max_len, True)
    plain = synth.synthesize(ph, pl, max_len=max_len, stop_threshold=0.5)
    assert synth.captures == 2 and plain["mel_lens"].tolist() == lens.tolist()
    out = synth.synthesize(ph, pl, max_len=max_len, stop_threshold=0.5, alignments=True)
    assert synth.captures == 3                   # the map-writing kernels are a capture of their own
    assert "alignments" not in plain
    for k in KEYS + ("mel_lens",):               # asking for the maps changes no other output bit
        assert torch.equal(out[k], plain[k]), k
    T = int(lens.max())
    H = cfg["decoder_n_head"]
    assert cfg["d_model"] // H == {"base": 64, "tiny1h": 128, "micro": 16}[cfg_name]
    assert len(out["alignments"]) == cfg["decoder_n_layers"]
    _assert_zero_behind(out, lens)
    ref = _oracle_alignments(_oracle64(cfg, w_seed, m), cfg, batch["phoneme"], batch["phoneme_lens"],
                             out["pred_melspec"].double().cpu())
    for i, (a, r) in enumerate(zip(out["alignments"], ref)):
        assert a.shape == (B, H, T, Tp) and a.dtype == torch.float32 and a.device == ph.device, (i, a.shape)
        r = r.clone()
        for b, n in enumerate(lens.tolist()):
            r[b, :, n:] = 0
            assert bool((a[b, :, :n, int(batch["phoneme_lens"][b]):] == 0).all()), (i, b)      # padded phonemes get no weight
            assert float((a[b, :, :n].double().sum(-1) - 1).abs().max()) <= 1e-5, (i, b)
        e = rel_l2(a, r)
        assert e < GATE, (cfg_name, i, e)


def test_alignments_are_the_training_forward_s():
    """dense phoneme lengths (the masked and the unmasked encoder coincide): the maps of the synthesized frames are what the
    eval-mode forward returns for them"""
    cfg, m, synth, batch, ph, pl, free, lens = _ragged_case("base", 141, 142, 3, 64, 24, False)
    out = synth.synthesize(ph, pl, max_len=24, stop_threshold=0.5, alignments=True)
    assert out["mel_lens"].tolist() == lens.tolist()
    m.eval()
    with torch.no_grad():
        fw = m(ph, out["pred_melspec"], pl, out["mel_lens"], need_alignments=True)
    assert len(fw["alignments"]) == len(out["alignments"])
    for i, (a, r) in enumerate(zip(out["alignments"], fw["alignments"])):
        assert a.shape == r.shape, (i, a.shape, r.shape)
        for b, n in enumerate(lens.tolist()):
            e = rel_l2(a[b, :, :n], r[b, :, :n])
            assert e < PATH_GATE, (i, b, e)


def test_state_hygiene_across_calls():
    from transformertts_amd.synthesis import Synthesizer
    cfg, m, synth, batch, ph, pl, free, lens = _ragged_case("base", 151, 152, 3, 50, 26, True)
    L = 26
    base_bytes = dict(synth.shape_bytes())
    long = synth.synthesize(ph, pl, max_len=L, stop_threshold=2.0, alignments=True)         # 25 frames of every row
    assert long["mel_lens"].tolist() == [L - 1] * 3 and synth.captures == 2      # __call__'s graph and the map-writing one
    key = next(iter(base_bytes))
    H, Tp_pad, cap = cfg["decoder_n_head"], key[1], key[2]
    assert synth.shape_bytes()[key] == base_bytes[key] + cfg["decoder_n_layers"] * 3 * H * cap * Tp_pad * 4
    # a short call on the same cached shape shows no frame, stop value or map row of the long one
    short = synth.synthesize(ph, pl, max_len=L, stop_threshold=0.5, alignments=True)
    assert short["mel_lens"].tolist() == lens.tolist() and len(synth.shape_bytes()) == 1
    _assert_zero_behind(short, lens)
    for b, n in enumerate(lens.tolist()):
        for k in ("pred_melspec", "pred_stop"):
            assert torch.equal(short[k][b, :n], long[k][b, :n]), (k, b)
        for a, al in zip(short["alignments"], long["alignments"]):
            assert torch.equal(a[b, :, :n], al[b, :, :n]), b
    # two identical calls are bitwise equal
    again = synth.synthesize(ph, pl, max_len=L, stop_threshold=0.5, alignments=True)
    for k in KEYS + ("mel_lens",):
        assert torch.equal(again[k], short[k]), k
    for a, b_ in zip(again["alignments"], short["alignments"]):
        assert torch.equal(a, b_)
    # alternating __call__ and synthesize on one Synthesizer leaves both correct
    for _ in range(2):
        f2 = synth(ph, pl, max_len=L, stop_threshold=2.0)
        for k in KEYS:
            assert torch.equal(f2[k], free[k]), k
        s2 = synth.synthesize(ph, pl, max_len=L, stop_threshold=0.5)
        for k in KEYS + ("mel_lens",):
            assert torch.equal(s2[k], short[k]), k
    # the all-rows stop of __call__ after per-row calls: it stops where every row is at or above the threshold at once
    p = torch.sigmoid(free["pred_stop"][..., 0].double()).cpu()
    allstop = (p >= 0.5).all(dim=0)
    n_all = int(allstop.double().argmax()) + 1 if bool(allstop.any()) else L - 1
    c = synth(ph, pl, max_len=L, stop_threshold=0.5)
    assert c["pred_melspec"].shape[1] == n_all >= int(lens.max())
    assert torch.equal(c["pred_melspec"], free["pred_melspec"][:, :n_all])
    # max_len, the threshold and the stop pattern changed all along: one graph per method (__call__, synthesize, synthesize
    # with maps) and nothing else
    assert synth.captures == 3
    other = synth.synthesize(ph, pl, max_len=L - 7, stop_threshold=0.4)
    assert int(other["mel_lens"].max()) <= L - 8
    other = synth.synthesize(ph, pl, max_len=L - 3, stop_threshold=0.6, alignments=True)
    assert synth.captures == 3 and synth.recaptures == 0 and len(synth.shape_bytes()) == 1
