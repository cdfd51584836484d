"""The attention window of batched synthesis (`Synthesizer.synthesize(window=AttentionWindow(...))`) and the kernels behind it
(csrc/decode.hip, ttts_decode_attention_window, ABI v21).

Kernel level, through the C ABI (B = 3, two heads of which head 0 is constrained, 130 keys with lengths 130 / 70 / 5, so that the
block boundaries at keys 63 | 64 and 127 | 128 are in play; NaN workspace, sentinel outputs, garbage positions): context and map
row against an fp64 masked softmax, exact zeros outside the window, the unconstrained head and a window that covers every key
against ttts_decode_attention_rows bit for bit, the position against the fp64 argmax (whose margin is asserted), ties, ended
rows, a launch without a guide.

Engine level (tiny, micro, base at B = 3, Tp = 70, max_len 24, stop heads refitted so that rows end at different frames): a
window wider than Tp against `synthesize(window=None)` bit for bit, narrow windows against an fp64 teacher-forced pass over the
engine's own frames whose windows are rebuilt from the returned positions (a free-running oracle would leave the engine's
trajectory for good at the first near-tie), structure of the positions, batch against B = 1, and state hygiene."""
import functools
from ctypes import c_void_p

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
GATE = 1e-4          # the engine against the fp64 oracle, as test_hip_synthesis_ragged.py
KERNEL_GATE = 1e-6   # one decode kernel against fp64, as test_hip_synthesis_ragged.py
MARGIN = 1e-3        # smallest distance of a stop probability from the threshold / between the two best scores a test relies on
SENT = 7.0           # what the output buffers hold before a kernel-level call
GARBAGE = 1234567    # what the positions hold before a kernel-level call
KEYS = ("pred_melspec", "post_melspec", "pred_stop")
B3, H2, TK = 3, 2, 130
LENS = (130, 70, 5)
ROWS, POS_LD = 6, 8
BIG = 2 ** 31 - 1


def _p(t, off=0):
    return c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def _state(t, row_end, t_end=POS_LD + 1):
    pad = [1] * (-len(row_end) % 4)
    st = torch.tensor([t, t_end, -1, 0] + list(row_end) + pad, dtype=torch.int64)
    st.view(torch.float32)[6] = 0.5
    st.view(torch.int32)[7] = 1
    return st.cuda()


def _window(back, ahead, guide_head, mask):
    w = torch.zeros(4, dtype=torch.int64)
    w.view(torch.int32)[:4] = torch.tensor([back, ahead, guide_head, 0], dtype=torch.int32)
    w[2] = mask
    return w.cuda()


@functools.lru_cache(maxsize=None)
def _operands(hd, seed=0):
    """q (B, d), memory K|V (B, TK, 2 d) with NaN behind each length: CPU fp32"""
    g = torch.Generator().manual_seed(500 + hd + seed)
    d = H2 * hd
    q = torch.randn(B3, d, generator=g)
    mem = torch.randn(B3, TK, 2 * d, generator=g)
    for b, L in enumerate(LENS):
        mem[b, L:] = float("nan")                                    # never read
    return q, mem


def _launch(hd, q, mem, t, centres, win, row_end=(-1, -1, -1), window_entry=True):
    """one cross-attention launch on sentinel-filled outputs: out (B, d), the map (B, H, ROWS, TK), pos (B, POS_LD) on the CPU"""
    from transformertts_amd import _lib, ops
    lib, s = _lib.load(), ops._stream()
    d = H2 * hd
    qd, memd = q.cuda(), mem.cuda()
    lens = torch.tensor(LENS, dtype=torch.int64).cuda()
    wsb = lib.ttts_decode_attention_workspace_bytes(B3, H2, hd, TK)
    ws = torch.full((wsb // 4,), float("nan"), device="cuda")
    out = torch.full((B3, d), SENT, device="cuda")
    amap = torch.full((B3, H2, ROWS, TK), SENT, device="cuda")
    pos = torch.full((B3, POS_LD), GARBAGE, dtype=torch.int32)
    if t >= 2:
        pos[:, t - 2] = torch.tensor(centres, dtype=torch.int32)
    pos = pos.cuda()
    st = _state(t, list(row_end))
    head = (_p(qd), d, _p(memd), _p(memd, d), 2 * d, TK * 2 * d, _p(lens), _p(out), d, _p(ws), wsb, B3, H2, hd, TK, _p(st, 8),
            _p(amap), ROWS * TK, TK, ROWS)
    if window_entry:
        _lib.check(lib.ttts_decode_attention_window(*head, _p(win), _p(pos), POS_LD, _p(st), s), "ttts_decode_attention_window")
    else:
        _lib.check(lib.ttts_decode_attention_rows(*head, _p(st), s), "ttts_decode_attention_rows")
    torch.cuda.synchronize()
    amap = amap.cpu()
    rest = torch.cat([amap[:, :, :t - 1], amap[:, :, t:]], dim=2)
    assert bool((rest == SENT).all())                                # only row t - 1 of the map is written
    return out.cpu(), amap[:, :, t - 1], pos.cpu()


def _bounds(c, back, ahead, L):
    return max(0, c - back), min(L - 1, c + ahead)


def _fp64(hd, q, mem, b, h, lo, hi):
    """scores (fp64, all keys below the length), weights and context of head h of row b over the keys lo .. hi"""
    d, L = H2 * hd, LENS[b]
    qh = q[b, h * hd:(h + 1) * hd].double() / hd ** 0.5
    sc = mem[b, :L, h * hd:(h + 1) * hd].double() @ qh
    masked = torch.full_like(sc, float("-inf"))
    masked[lo:hi + 1] = sc[lo:hi + 1]
    a = torch.softmax(masked, dim=0)
    return sc, a, a @ mem[b, :L, d + h * hd:d + (h + 1) * hd].double()


# (frame, centre per row (ignored at frame 1: the positions hold garbage there and the centre is 0), back, ahead)
CASES = [
    (1, (0, 0, 0), 1, 3),            # centres at 0 without reading them
    (2, (63, 63, 4), 1, 3),          # the window straddles keys 63 | 64; row 2 at len - 1
    (3, (64, 64, 0), 2, 2),          # ... from the other side
    (4, (129, 69, 3), 1, 3),         # centres at len - 1: c + ahead is past the length
    (5, (127, 60, 2), 3, 5),         # keys 127 | 128, and c + ahead past the length in rows 0 and 2
    (6, (100, 66, 1), 70, 70),       # three blocks in one window
    (2, (64, 63, 4), 0, 0),          # one key: the map row is one 1.0 and the context is that key's value row
]


def _case_windows(t, centres, back, ahead):
    return [_bounds(0 if t == 1 else c, back, ahead, L) for c, L in zip(centres, LENS)]


def test_the_reference_separates_the_two_best_scores_of_every_case():
    """(CPU arithmetic only) what lets the position test ask for equality: in every window the fp64 scores' two largest are at
    least 1e-3 apart"""
    for hd in (16, 64, 128):
        q, mem = _operands(hd)
        for t, centres, back, ahead in CASES:
            for b, (lo, hi) in enumerate(_case_windows(t, centres, back, ahead)):
                sc, _, _ = _fp64(hd, q, mem, b, 0, lo, hi)
                top = sc[lo:hi + 1].sort(descending=True).values
                assert top.numel() == 1 or float(top[0] - top[1]) >= MARGIN, (hd, t, b, float(top[0] - top[1]))


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_window_kernels_vs_fp64_masked_softmax(hd):
    q, mem = _operands(hd)
    d = H2 * hd
    rows_out, rows_map, _ = _launch(hd, q, mem, 2, (0, 0, 0), None, window_entry=False)
    assert not bool((rows_out == SENT).any())
    for t, centres, back, ahead in CASES:
        win = _window(back, ahead, 0, 1)                             # head 0 constrained and the guide, head 1 free
        out, row, pos = _launch(hd, q, mem, t, centres, win)
        for b, (lo, hi) in enumerate(_case_windows(t, centres, back, ahead)):
            L = LENS[b]
            sc, a, ctx = _fp64(hd, q, mem, b, 0, lo, hi)
            e_a, e_c = rel_l2(row[b, 0, :L], a), rel_l2(out[b, :hd], ctx)
            print(f"hd {hd} t {t} row {b} window [{lo}, {hi}]: map {e_a:.2e} context {e_c:.2e}")
            assert e_a <= KERNEL_GATE and e_c <= KERNEL_GATE, (hd, t, b, e_a, e_c)
            assert bool((row[b, 0, :lo] == 0).all()) and bool((row[b, 0, hi + 1:] == 0).all()), (hd, t, b)   # up to max_keys
            assert abs(float(row[b, 0].double().sum()) - 1) <= 1e-6
            # the free head: what the entry point without a window gives, bit for bit
            assert torch.equal(out[b, hd:], rows_out[b, hd:]) and torch.equal(row[b, 1], rows_map[b, 1]), (hd, t, b)
            # the position: the fp64 argmax inside the window (its margin is asserted here and in the CPU test above)
            top = sc[lo:hi + 1].sort(descending=True).values
            assert top.numel() == 1 or float(top[0] - top[1]) >= MARGIN
            assert int(pos[b, t - 1]) == lo + int(sc[lo:hi + 1].argmax()), (hd, t, b, int(pos[b, t - 1]))
            if lo == hi:
                assert row[b, 0].tolist() == [1.0 if j == lo else 0.0 for j in range(TK)]
                assert torch.equal(out[b, :hd], mem[b, lo, d:d + hd]), (hd, b)
        keep = torch.ones(POS_LD, dtype=torch.bool)
        keep[t - 1] = False
        if t >= 2:
            assert pos[:, t - 2].tolist() == list(centres)
            keep[t - 2] = False
        assert bool((pos[:, keep] == GARBAGE).all())                 # nothing else of the positions is written


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_a_window_over_every_key_is_the_kernel_without_one(hd):
    q, mem = _operands(hd)
    rows_out, rows_map, _ = _launch(hd, q, mem, 3, (0, 0, 0), None, window_entry=False)
    for t, centres, back, ahead in ((3, (0, 69, 2), TK, TK), (1, (0, 0, 0), BIG, BIG), (3, (129, 0, 4), BIG, BIG)):
        out, row, pos = _launch(hd, q, mem, t, centres, _window(back, ahead, 1, 3))          # both heads, head 1 the guide
        assert torch.equal(out, rows_out) and torch.equal(row, rows_map), (hd, t)            # (a frame's map row is row t - 1)
        for b, L in enumerate(LENS):                                 # the guide sees every key below the length
            sc, _, _ = _fp64(hd, q, mem, b, 1, 0, L - 1)
            top = sc.sort(descending=True).values
            assert float(top[0] - top[1]) >= MARGIN
            assert int(pos[b, t - 1]) == int(sc.argmax()), (hd, b)


def _tie_operands(hd, keys):
    """row 0's keys `keys` all hold the same bits, along head 0's query: far above every other score of the head"""
    q, mem = _operands(hd, seed=1)
    q, mem = q.clone(), mem.clone()
    for j in keys:
        mem[0, j, :hd] = 3.0 * q[0, :hd]
    return q, mem


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_ties_ended_rows_and_a_launch_without_a_guide(hd):
    # (keys that tie, centre, back, ahead): one wave of a block, two waves of a block, two blocks
    for keys, c, back, ahead in (((65, 67), 66, 2, 2), ((70, 90), 80, 12, 12), ((60, 66), 63, 4, 4), ((66, 60, 127, 128), 90, 40, 40)):
        q, mem = _tie_operands(hd, keys)
        sc, _, _ = _fp64(hd, q, mem, 0, 0, 0, LENS[0] - 1)
        others = torch.ones(LENS[0], dtype=torch.bool)
        others[list(keys)] = False
        assert float(sc[keys[0]] - sc[others].max()) >= 1.0 and len(set(sc[list(keys)].tolist())) == 1
        out, row, pos = _launch(hd, q, mem, 2, (c, 0, 0), _window(back, ahead, 0, 1))
        assert int(pos[0, 1]) == min(keys), (hd, keys, int(pos[0, 1]))
        w = row[0, 0, list(keys)]
        assert bool((w == w[0]).all()) and float(w[0]) > 0           # equal scores, equal weights
    # an ended row writes neither output, map nor position; the running rows are what they are with no row ended
    q, mem = _operands(hd)
    win = _window(1, 3, 0, 1)
    ref_out, ref_row, ref_pos = _launch(hd, q, mem, 2, (63, 63, 4), win)
    out, row, pos = _launch(hd, q, mem, 2, (63, 63, 4), win, row_end=(-1, 5, 0))
    assert bool((out[1] == SENT).all()) and bool((row[1] == SENT).all()) and int(pos[1, 1]) == GARBAGE
    for b in (0, 2):
        assert torch.equal(out[b], ref_out[b]) and torch.equal(row[b], ref_row[b]) and int(pos[b, 1]) == int(ref_pos[b, 1])
    # no guide in this layer: the window still holds, the positions are left alone
    out, row, pos = _launch(hd, q, mem, 2, (63, 63, 4), _window(1, 3, -1, 1))
    assert torch.equal(out, ref_out) and torch.equal(row, ref_row)
    assert pos[:, 0].tolist() == [63, 63, 4] and bool((pos[:, 1:] == GARBAGE).all())


# ------------------------------------------------------------------------------------------------------------ the engine
B, TP, MAX_LEN = 3, 70, 24
SEEDS = {"tiny": (171, 172), "micro": (173, 174), "base": (175, 176)}
GUIDE = {"tiny": (1, 0), "micro": (0, 1), "base": (1, 2)}


def _helpers():
    import test_hip_synthesis_ragged as r
    return r


def _fit(m, synth, ph, pl, window):
    """refit the stop head on the frames this window decodes (the stop head does not feed back): ramps crossing at spread
    frames.  -> the free-running call (threshold 2.0) and each row's end at threshold 0.5, its margin asserted"""
    r = _helpers()
    F = MAX_LEN - 1
    probe = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=2.0, window=window)
    cross = [max(2, round(F * (b + 1) / (B + 0.5))) for b in range(B)]
    r._fit_stop_head(m, probe["pred_melspec"], r._ramps(cross, F))
    free = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=2.0, alignments=True, window=window)
    assert torch.equal(free["pred_melspec"], probe["pred_melspec"])
    p = torch.sigmoid(free["pred_stop"][..., 0].double()).cpu()
    lens, margin = r._first_crossings(p, 0.5, MAX_LEN)
    print(f"window {window}: target ends {cross}, engine ends {lens.tolist()}, margin {margin:.4f}")
    assert margin >= MARGIN, margin
    assert len(set(lens.tolist())) > 1                               # the rows do end at different frames
    return free, lens


@functools.lru_cache(maxsize=None)
def _model_case(cfg_name):
    from transformertts_amd.synthesis import Synthesizer
    r = _helpers()
    cfg, m = r._build(cfg_name, SEEDS[cfg_name][0])
    batch, ph, pl = r._batch(cfg, B, TP, SEEDS[cfg_name][1])
    return cfg, m, Synthesizer(m), batch, ph, pl


def _constrained(cfg, window):
    L, H = cfg["decoder_n_layers"], cfg["decoder_n_head"]
    layers = range(L) if window.layers is None else window.layers
    heads = range(H) if window.heads is None else window.heads
    return [(i, h) for i in layers for h in heads]


def _oracle_window_pass(sd, cfg, phoneme, phoneme_lens, pred, windows, constrained):
    """fp64 teacher-forced decoder pass over the frames `pred` (B, T, n_mels) on the unmasked-encoder memory, from the oracle's
    blocks as oracle_inference puts them together; the cross-attention scores of the (layer, head)s in `constrained` are -inf
    outside windows[b][f] = (lo, hi).  -> maps per layer, mel frames, stop logits"""
    import math
    import torch.nn.functional as F
    from oracle.ref_model import _ffn, _ln, conv_norm_bn, encoder_layer, multi_head_attention, positional_encoding
    Bn, T = pred.shape[:2]
    Tp = phoneme.size(1)
    x = F.embedding(phoneme, sd["emb.weight"])
    for i in range(cfg["encoder_prenet_n_layers"]):
        x = conv_norm_bn(sd, f"enc_prenet.layers.{2 * i}", x, False, False)
    x = F.linear(x, sd["enc_prenet.linear.linear.weight"], sd["enc_prenet.linear.linear.bias"])
    x = positional_encoding(sd, x, 0.1, False)
    full = torch.full((Bn,), Tp, dtype=torch.long)
    for i in range(cfg["encoder_n_layers"]):
        x = encoder_layer(sd, f"encoder.layers.{i}", x, cfg["encoder_n_head"], full, cfg["encoder_dropout"], False)
    mem = x
    y = torch.cat([torch.zeros_like(pred[:, :1]), pred[:, :-1]], dim=1)
    y = F.relu(F.linear(y, sd["dec_prenet.linear1.linear.weight"], sd["dec_prenet.linear1.linear.bias"]))
    y = F.relu(F.linear(y, sd["dec_prenet.linear2.linear.weight"], sd["dec_prenet.linear2.linear.bias"]))
    y = positional_encoding(sd, y, 0.1, False)
    lens_t = torch.full((Bn,), T, dtype=torch.long)
    H = cfg["decoder_n_head"]
    d = y.size(-1)
    hd = d // H
    keys = torch.arange(Tp).view(1, 1, Tp)
    outside = torch.zeros(Bn, T, Tp, dtype=torch.bool)
    for b in range(Bn):
        for f in range(T):
            lo, hi = windows[b][f]
            outside[b, f] = (torch.arange(Tp) < lo) | (torch.arange(Tp) > hi)
    maps = []
    for i in range(cfg["decoder_n_layers"]):
        pre = f"decoder.layers.{i}"
        sa, _ = multi_head_attention(sd, f"{pre}.self_attn", y, y, H, lens_t, True, 0.0, False)
        y = _ln(sd, f"{pre}.norm1", y + sa)
        # the cross-attention of ref_model.multi_head_attention with the window on the constrained heads
        w_in, b_in = sd[f"{pre}.multihead_attn.in_proj_weight"], sd[f"{pre}.multihead_attn.in_proj_bias"]
        qh = F.linear(y, w_in[:d], b_in[:d]).view(Bn, T, H, hd).transpose(1, 2) * math.sqrt(1.0 / hd)
        kh = F.linear(mem, w_in[d:2 * d], b_in[d:2 * d]).view(Bn, Tp, H, hd).transpose(1, 2)
        vh = F.linear(mem, w_in[2 * d:], b_in[2 * d:]).view(Bn, Tp, H, hd).transpose(1, 2)
        s = qh @ kh.transpose(-1, -2)
        dead = (keys >= phoneme_lens.view(Bn, 1, 1)).unsqueeze(1).expand(Bn, H, T, Tp).clone()
        for h in range(H):
            if (i, h) in constrained:
                dead[:, h] |= outside
        a = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
        o = (a @ vh).transpose(1, 2).reshape(Bn, T, d)
        ca = F.linear(o, sd[f"{pre}.multihead_attn.out_proj.weight"], sd[f"{pre}.multihead_attn.out_proj.bias"])
        y = _ln(sd, f"{pre}.norm2", y + ca)
        y = _ln(sd, f"{pre}.norm3", y + _ffn(sd, pre, y, 0.0, False))
        maps.append(a)
    mel = F.linear(y, sd["linear1.linear.weight"], sd["linear1.linear.bias"])
    stop = F.linear(y, sd["linear2.linear.weight"], sd["linear2.linear.bias"])
    return maps, mel, stop


def _oracle_postnet(sd, cfg, mel):
    from oracle.ref_model import conv_norm_bn
    z = mel
    n_post = cfg["postnet_n_layers"]
    for i in range(n_post):
        z = conv_norm_bn(sd, f"postnet.layers.{3 * i}", z, False, False)
        if i < n_post - 1:
            z = torch.tanh(z)
    return z + mel


def _windows_from_positions(positions, mel_lens, ph_lens, window):
    """per row, per frame (lo, hi): the positions shifted by one frame and starting at 0; behind a row's end the whole row"""
    out = []
    for b in range(positions.shape[0]):
        n, L = int(mel_lens[b]), int(ph_lens[b])
        row = []
        for f in range(positions.shape[1]):
            c = 0 if f == 0 else int(positions[b, f - 1])
            row.append(_bounds(c, window.back, window.ahead, L) if f < n else (0, L - 1))
        out.append(row)
    return out


def _check_positions(out, pl, window):
    pos, lens = out["attention_positions"].cpu(), out["mel_lens"].tolist()
    assert out["attention_positions"].dtype == torch.int64 and out["attention_positions"].device == pl.device
    assert tuple(pos.shape) == (B, max(lens))
    for b, n in enumerate(lens):
        assert bool((pos[b, n:] == -1).all()), b
        prev = 0                                                     # the first window is centred at 0
        for f in range(n):
            c = int(pos[b, f])
            assert 0 <= c < int(pl[b]) and -window.back <= c - prev <= window.ahead, (b, f, prev, c)
            prev = c
    return pos


@pytest.mark.parametrize("cfg_name", ["tiny", "micro", "base"])
def test_a_window_wider_than_the_phonemes_changes_no_bit(cfg_name):
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m, _, batch, ph, pl = _model_case(cfg_name)
    assert cfg["d_model"] // cfg["decoder_n_head"] == {"tiny": 64, "micro": 16, "base": 64}[cfg_name]
    synth = Synthesizer(m)
    wide = AttentionWindow(GUIDE[cfg_name], TP + 1, TP + 1)
    _fit(m, synth, ph, pl, None)
    c0 = synth.captures
    plain = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=0.5, alignments=True)
    assert synth.captures == c0                                      # (the fit ran the map-writing graph already)
    a = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=0.5, window=wide)
    assert synth.captures == c0 + 1                                  # asking for a window: one graph ...
    out = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=0.5, alignments=True, window=wide)
    assert synth.captures == c0 + 2                                  # ... and a second one only with maps
    assert len(set(plain["mel_lens"].tolist())) > 1
    for k in KEYS + ("mel_lens",):
        assert torch.equal(out[k], plain[k]) and torch.equal(a[k], plain[k]), k
    for x, y in zip(out["alignments"], plain["alignments"]):
        assert torch.equal(x, y)
    assert "alignments" not in a and torch.equal(a["attention_positions"], out["attention_positions"])
    pos = _check_positions(out, pl, wide)
    gl, gh = GUIDE[cfg_name]
    for b, n in enumerate(out["mel_lens"].tolist()):
        for f in range(n):
            row = out["alignments"][gl][b, gh, f]
            assert float(row.max() - row[int(pos[b, f])]) <= 1e-7, (b, f)
    assert "attention_positions" not in plain
    synth.synthesize(ph, pl, max_len=MAX_LEN - 2, stop_threshold=0.4, window=AttentionWindow((0, 0), 0, 2, layers=[0], heads=[0]))
    assert synth.captures == c0 + 2 and synth.recaptures == 0        # another window, guide and selection: data


def _subset(cfg, cfg_name):
    """a strict subset of the (layer, head)s that contains the guide"""
    gl, gh = GUIDE[cfg_name]
    if cfg["decoder_n_layers"] > 1:
        return dict(layers=[gl], heads=[gh])
    return dict(heads=[gh])


@pytest.mark.parametrize("cfg_name,subset", [("tiny", False), ("tiny", True), ("micro", False), ("micro", True),
                                             ("base", False), ("base", True)])
def test_narrow_window_vs_fp64_teacher_forced_pass(cfg_name, subset):
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    r = _helpers()
    cfg, m, _, batch, ph, pl = _model_case(cfg_name)
    synth = Synthesizer(m)
    window = AttentionWindow(GUIDE[cfg_name], 1, 3, **(_subset(cfg, cfg_name) if subset else {}))
    constrained = _constrained(cfg, window)
    L, H = cfg["decoder_n_layers"], cfg["decoder_n_head"]
    assert GUIDE[cfg_name] in constrained and (len(constrained) < L * H) == subset
    free, lens = _fit(m, synth, ph, pl, window)
    out = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=0.5, alignments=True, window=window)
    assert out["mel_lens"].tolist() == lens.tolist()
    T = int(lens.max())
    r._assert_zero_behind(out, lens)
    pos = _check_positions(out, pl, window)
    ph_lens = batch["phoneme_lens"]
    windows = _windows_from_positions(pos, lens, ph_lens, window)
    sd = r._oracle64(cfg, SEEDS[cfg_name][0], m)
    maps, mel, stop = _oracle_window_pass(sd, cfg, batch["phoneme"], ph_lens, out["pred_melspec"].double().cpu(), windows,
                                          constrained)
    gl, gh = GUIDE[cfg_name]
    free_outside = False
    for i, (a, ref) in enumerate(zip(out["alignments"], maps)):
        assert a.shape == (B, H, T, TP) and a.dtype == torch.float32
        ref = ref.clone()
        a64 = a.double().cpu()
        for b, n in enumerate(lens.tolist()):
            ref[b, :, n:] = 0
            assert float((a64[b, :, :n].sum(-1) - 1).abs().max()) <= 1e-5, (i, b)
            assert bool((a64[b, :, :n, int(ph_lens[b]):] == 0).all()), (i, b)
            for h in range(H):
                for f in range(n):
                    lo, hi = windows[b][f]
                    w_out = float(a64[b, h, f, :lo].sum() + a64[b, h, f, hi + 1:].sum())
                    if (i, h) in constrained:
                        assert w_out == 0.0, (i, b, h, f)            # exact zeros outside the window
                    else:
                        free_outside |= w_out > 0
        e = rel_l2(a64, ref)
        print(f"{cfg_name} subset {subset} layer {i}: maps rel-L2 {e:.2e}")
        assert e < GATE, (cfg_name, i, e)
    assert free_outside == subset                                    # the selection selects
    # the trajectory: at every frame the oracle's guide weight at the engine's position is its largest in-window weight
    worst = 0.0
    for b, n in enumerate(lens.tolist()):
        for f in range(n):
            row = maps[gl][b, gh, f]
            worst = max(worst, float(row.max() - row[int(pos[b, f])]))
    print(f"{cfg_name} subset {subset}: trajectory gap {worst:.2e}")
    assert worst <= 1e-4, worst
    for b, n in enumerate(lens.tolist()):
        want = {"pred_melspec": mel[b, :n], "pred_stop": stop[b, :n],
                "post_melspec": _oracle_postnet(sd, cfg, mel[b:b + 1, :n])[0]}
        for k in KEYS:
            e = rel_l2(out[k][b, :n], want[k])
            assert e < GATE, (cfg_name, b, k, e)


@pytest.mark.parametrize("cfg_name", ["tiny", "base"])
def test_structure_of_the_positions(cfg_name):
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    r = _helpers()
    cfg, m, _, batch, ph, pl = _model_case(cfg_name)
    synth = Synthesizer(m)
    H = cfg["decoder_n_head"]
    for window in (AttentionWindow(GUIDE[cfg_name], 0, 2), AttentionWindow(GUIDE[cfg_name], 0, 0)):
        free, lens = _fit(m, synth, ph, pl, window)
        out = synth.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=0.5, alignments=True, window=window)
        assert out["mel_lens"].tolist() == lens.tolist()
        r._assert_zero_behind(out, lens)                             # everything behind mel_lens is 0 ...
        pos = _check_positions(out, pl, window)                      # ... and the positions there are -1
        for b, n in enumerate(lens.tolist()):
            steps = pos[b, 1:n] - pos[b, :n - 1]
            assert bool((steps >= 0).all()), b                       # back = 0: the positions never decrease
            if window.ahead == 0:
                assert bool((pos[b, :n] == 0).all())
                for a in out["alignments"]:                          # every head is constrained: one-hot at key 0
                    want = torch.zeros(H, n, TP, device=a.device)
                    want[:, :, 0] = 1.0
                    assert torch.equal(a[b, :, :n], want), b
    assert synth.captures == 2                                       # the window graph and the window + maps graph


@pytest.mark.parametrize("cfg_name", ["tiny", "micro", "base"])
def test_a_row_of_a_batch_is_its_own_call(cfg_name):
    """A row of a batched windowed call is, bit for bit, the B = 1 windowed call of that utterance -- wherever the engine gives
    the decode kernels the same memory in both calls.  The encoder and the memory K/V projection run once per call on the `ops`
    path, whose fp16x3 GEMMs pre-scale an operand by the largest magnitude of the whole batch: measured on an MI355X, tiny and
    micro hand every row the same K/V bits at B = 1 and B = 3, base does so for row 0 only (rows 1 and 2: K/V rel-L2 3.4e-07
    and 2.9e-07 apart, `synthesize(window=None)` 2.4e-07 apart -- without any window code; tests/test_hip_synthesis.py holds
    that path to 1e-5 across batches).  So: tiny and micro must be bitwise in every row; a base row whose unwindowed call is
    bitwise its B = 1 call must be bitwise with the window too, and the other rows stay inside that 1e-5."""
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m, _, batch, ph, pl = _model_case(cfg_name)
    synth = Synthesizer(m)
    window = AttentionWindow(GUIDE[cfg_name], 1, 3)
    free, lens = _fit(m, synth, ph, pl, window)

    def call(p, l, w):
        return synth.synthesize(p, l, max_len=MAX_LEN, stop_threshold=0.5, alignments=True, window=w)

    out, plain = call(ph, pl, window), call(ph, pl, None)
    bitwise = 0
    for b, n in enumerate(lens.tolist()):
        alone, alone_plain = call(ph[b:b + 1], pl[b:b + 1], window), call(ph[b:b + 1], pl[b:b + 1], None)
        k = int(plain["mel_lens"][b])
        same_memory = (alone_plain["mel_lens"].tolist() == [k] and
                       torch.equal(alone_plain["pred_melspec"][0], plain["pred_melspec"][b, :k]) and
                       all(torch.equal(x[0], y[b, :, :k]) for x, y in zip(alone_plain["alignments"], plain["alignments"])))
        print(f"{cfg_name} row {b}: the unwindowed call is bitwise its B = 1 call: {same_memory}")
        assert alone["mel_lens"].tolist() == [n], (b, n, alone["mel_lens"].tolist())
        if same_memory:
            bitwise += 1
            assert torch.equal(alone["attention_positions"][0], out["attention_positions"][b, :n]), b
            for key in KEYS:
                assert torch.equal(alone[key][0], out[key][b, :n]), (key, b)
            for x, y in zip(alone["alignments"], out["alignments"]):
                assert torch.equal(x[0], y[b, :, :n]), b
        else:
            for key in KEYS:
                e = rel_l2(alone[key][0], out[key][b, :n])
                assert e < 1e-5, (key, b, e)
    assert bitwise == B or cfg_name == "base", bitwise


def test_state_hygiene_across_windows():
    from transformertts_amd.synthesis import AttentionWindow, Synthesizer
    cfg, m, _, batch, ph, pl = _model_case("base")
    w1 = AttentionWindow(GUIDE["base"], 1, 3)
    w2 = AttentionWindow((0, 1), 0, 2, layers=(0, 2), heads=(1, 3))
    synth = Synthesizer(m)
    _fit(m, synth, ph, pl, w1)

    def call(s, w, maps=False):
        return s.synthesize(ph, pl, max_len=MAX_LEN, stop_threshold=0.5, alignments=maps, window=w)

    def same(x, y):
        assert set(x) == set(y)
        for k in x:
            if k == "alignments":
                assert all(torch.equal(i, j) for i, j in zip(x[k], y[k]))
            else:
                assert torch.equal(x[k], y[k]), k

    fresh = {(w, maps): call(Synthesizer(m), w, maps) for w in (None, w1, w2) for maps in (False, True)}
    assert not torch.equal(fresh[(w1, False)]["pred_melspec"], fresh[(None, False)]["pred_melspec"])     # the window does act
    assert not torch.equal(fresh[(w1, False)]["attention_positions"], fresh[(w2, False)]["attention_positions"])
    synth = Synthesizer(m)
    same(call(synth, None), fresh[(None, False)])
    same(call(synth, w1), fresh[(w1, False)])
    assert synth.captures == 2
    key = next(iter(synth.shape_bytes()))
    assert key == (B, 128, 256)
    before = synth.shape_bytes()[key]
    L, H, d, nm, dff = cfg["decoder_n_layers"], cfg["decoder_n_head"], cfg["d_model"], cfg["n_mels"], cfg["decoder_d_ffn"]
    cap, tp_pad = key[2], key[1]
    ws = max(B * H * -(-cap // 64) * (d // H + 4) * 4, 16)
    want = ((4 + 4) * 8 + B * cap * nm * 4 + B * cap * 4 + 4 * B * d * 4 + B * dff * 4 + L * B * cap * 2 * d * 4 +
            L * B * tp_pad * 2 * d * 4 + B * 8 + ws + L * 32 + B * cap * 4)          # ... the window structs and `pos` last
    assert before == want, (before, want)
    for _ in range(2):                                               # alternating kinds and windows on one Synthesizer
        same(call(synth, w2), fresh[(w2, False)])
        same(call(synth, None), fresh[(None, False)])
        same(call(synth, w1), fresh[(w1, False)])
        assert synth.captures == 2 and synth.shape_bytes()[key] == before
    same(call(synth, w1, True), fresh[(w1, True)])
    same(call(synth, None, True), fresh[(None, True)])
    assert synth.captures == 4
    assert synth.shape_bytes()[key] == before + L * B * H * cap * tp_pad * 4
    for _ in range(2):
        same(call(synth, w2, True), fresh[(w2, True)])
        same(call(synth, w1), fresh[(w1, False)])
        same(call(synth, None, True), fresh[(None, True)])
        same(call(synth, w1, True), fresh[(w1, True)])
    assert synth.captures == 4 and synth.recaptures == 0 and len(synth.shape_bytes()) == 1
