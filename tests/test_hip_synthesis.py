"""The graph-replayed synthesizer (transformertts_amd/synthesis.py) and its decode kernels (csrc/decode.hip): every kernel
against fp64 through the C ABI, the whole engine against the reference's own inference output, the fp64 oracle loop,
`model.inference` and the teacher-forced forward, its stop semantics, reproducibility, weight following and batch
independence."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
GATE = 1e-4          # outputs against the fp64 oracle, as test_hip_model.py
KERNEL_GATE = 1e-6   # one decode kernel against fp64
NAN = float("nan")


def _p(t, off=0):
    return c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def _state(t, t_end=1 << 40, thr=0.5, stop=-1):
    st = torch.tensor([t, t_end, stop, 0], dtype=torch.int64)
    st.view(torch.float32)[6] = thr
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


def _oracle64(cfg, w_seed):
    from oracle import fill_state
    sd = fill_state(cfg, w_seed)
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _batch(cfg, B, Tp, seed, ragged=True):
    from oracle import synth_batch
    b = synth_batch(B, Tp, 40, cfg["n_mels"], cfg["n_phon"], ragged=ragged, seed=seed)
    return b, b["phoneme"].cuda(), b["phoneme_lens"].cuda()


KEYS = ("pred_melspec", "post_melspec", "pred_stop")


# ------------------------------------------------------------------------------------------------ kernels vs fp64
@pytest.mark.parametrize("M", [1, 5, 64])
def test_decode_linear_vs_fp64(M):
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(100 + M)
    st = _state(7)
    for N, K in [(1, 256), (80, 256), (256, 80), (768, 256), (1024, 256), (256, 1024), (1536, 512)]:
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g)
        r = torch.randn(M, N, generator=g)
        xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), r.cuda()
        base = x.double() @ w.double().T + b.double()
        for act, res in ((0, False), (1, False), (0, True), (1, True)):
            want = (base.clamp_min(0) if act else base) + (r.double() if res else 0)
            y = torch.full((M, N), NAN, device="cuda")
            _lib.check(lib.ttts_decode_linear(_p(xd), K, 0, _p(wd), _p(bd), _p(rd) if res else None, N, _p(y), N, 0, None, 0, 0,
                                              N, M, N, K, act, _p(st), s), "ttts_decode_linear")
            torch.cuda.synchronize()
            assert rel_l2(y, want) <= KERNEL_GATE, (M, N, K, act, res, rel_l2(y, want))
    # the self-attention in-projection form: x read at row t - 1 of a (M, T, K) buffer, q columns to y, K/V columns into row
    # t - 1 of a (M, cap, 2d) cache, t taken from the state block; nothing else of the cache is written
    d, T, cap, t = 256, 9, 12, 7
    x = torch.randn(M, T, d, generator=g)
    w = torch.randn(3 * d, d, generator=g) / d ** 0.5
    b = torch.randn(3 * d, generator=g)
    want = x[:, t - 1].double() @ w.double().T + b.double()
    y = torch.full((M, d), NAN, device="cuda")
    cache = torch.full((M, cap, 2 * d), 7.0, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    _lib.check(lib.ttts_decode_linear(_p(xd), T * d, d, _p(wd), _p(bd), None, 0, _p(y), d, 0, _p(cache),
                                      cap * 2 * d, 2 * d, d, M, 3 * d, d, 0, _p(st), s), "ttts_decode_linear")
    torch.cuda.synchronize()
    assert rel_l2(y, want[:, :d]) <= KERNEL_GATE
    assert rel_l2(cache[:, t - 1], want[:, d:]) <= KERNEL_GATE
    others = torch.cat([cache[:, :t - 1], cache[:, t:]], dim=1)
    assert bool((others == 7.0).all())
    # a finished decode (stop recorded, or t at t_end) leaves every output untouched
    for done in (_state(7, stop=3), _state(7, t_end=7)):
        y2 = torch.full((M, d), 5.0, device="cuda")
        _lib.check(lib.ttts_decode_linear(_p(xd), T * d, d, _p(wd), _p(bd), None, 0, _p(y2), d, 0, _p(cache),
                                          cap * 2 * d, 2 * d, d, M, 3 * d, d, 0, _p(done), s), "ttts_decode_linear")
        torch.cuda.synchronize()
        assert bool((y2 == 5.0).all())


def _attn_ref(q, k, v, lens, H, hd):
    """fp64: q (B, H*hd), k / v (B, Tk, H*hd), keys < lens[b]"""
    B = q.shape[0]
    out = torch.zeros(B, H * hd, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        qh = q[b].double().view(H, hd) / hd ** 0.5
        kh = k[b, :L].double().view(L, H, hd).transpose(0, 1)
        vh = v[b, :L].double().view(L, H, hd).transpose(0, 1)
        p = torch.softmax(torch.einsum("hd,hkd->hk", qh, kh), dim=-1)
        out[b] = torch.einsum("hk,hkd->hd", p, vh).reshape(-1)
    return out


@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_decode_attention_vs_fp64(hd):
    """self-attention over the first t cache rows (t from the state block) and cross-attention with ragged lengths; rows at or
    past a length hold NaN, and the output is finite and bit-identical to a run with finite values there"""
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(hd)
    H = 256 // hd if hd < 128 else 2
    d = H * hd
    B, cap = 2, 1536
    ws = torch.zeros(lib.ttts_decode_attention_workspace_bytes(B + 1, H, hd, cap) // 4, device="cuda")
    cache = torch.randn(B, cap, 2 * d, generator=g).cuda()
    q = torch.randn(B, d, generator=g).cuda()
    for t in (1, 2, 63, 64, 65, 777, 1499):
        st = _state(t)
        outs = []
        for fill in (NAN, 3.0):
            c = cache.clone()
            c[:, t:] = fill
            out = torch.full((B, d), NAN, device="cuda")
            _lib.check(lib.ttts_decode_attention(_p(q), d, _p(c), _p(c, d), 2 * d, cap * 2 * d, None, _p(out), d, _p(ws),
                                                 ws.numel() * 4, B, H, hd, cap, _p(st), s), "ttts_decode_attention")
            torch.cuda.synchronize()
            outs.append(out)
        want = _attn_ref(q.cpu(), cache[:, :, :d].cpu(), cache[:, :, d:].cpu(), [t] * B, H, hd)
        assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1]), t
        assert rel_l2(outs[0], want) <= KERNEL_GATE, (hd, t, rel_l2(outs[0], want))
    # cross-attention: memory K/V (B, Tk, 2d) with ragged lengths
    B, Tk = 3, 200
    lens = torch.tensor([200, 77, 1], dtype=torch.int64)
    mem = torch.randn(B, Tk, 2 * d, generator=g)
    q = torch.randn(B, d, generator=g).cuda()
    st = _state(5)
    lens_d = lens.cuda()
    outs = []
    for fill in (NAN, -2.0):
        mk = mem.clone()
        for b in range(B):
            mk[b, int(lens[b]):] = fill
        mk = mk.cuda()
        out = torch.full((B, d), NAN, device="cuda")
        _lib.check(lib.ttts_decode_attention(_p(q), d, _p(mk), _p(mk, d), 2 * d, Tk * 2 * d, _p(lens_d), _p(out), d, _p(ws),
                                             ws.numel() * 4, B, H, hd, Tk, _p(st), s), "ttts_decode_attention")
        torch.cuda.synchronize()
        outs.append(out)
    want = _attn_ref(q.cpu(), mem[:, :, :d], mem[:, :, d:], lens, H, hd)
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    assert rel_l2(outs[0], want) <= KERNEL_GATE, (hd, rel_l2(outs[0], want))


def test_decode_frame_in_out_and_layernorm_vs_fp64():
    from transformertts_amd import _lib
    lib, s = _lib_stream()
    g = torch.Generator().manual_seed(9)
    B, d, nm, cap, t = 5, 256, 80, 40, 13
    ys = torch.randn(B, cap, nm, generator=g)
    w1, b1 = torch.randn(d, nm, generator=g) / nm ** 0.5, torch.randn(d, generator=g)
    w2, b2 = torch.randn(d, d, generator=g) / d ** 0.5, torch.randn(d, generator=g)
    pe, alpha = torch.randn(100, d, generator=g), torch.tensor([0.7])
    st = _state(t, thr=0.5)
    tmp, out = torch.zeros(B, d, device="cuda"), torch.full((B, d), NAN, device="cuda")
    ysd = ys.cuda()
    dev = [t_.cuda() for t_ in (w1, b1, w2, b2, pe, alpha)]
    _lib.check(lib.ttts_decode_frame_in(_p(ysd), cap * nm, nm, *[_p(t_) for t_ in dev], _p(tmp), _p(out), B, d, _p(st), s),
               "ttts_decode_frame_in")
    h1 = (ys[:, t - 1].double() @ w1.double().T + b1.double()).clamp_min(0)
    want = (h1 @ w2.double().T + b2.double()).clamp_min(0) + 0.7 * pe[t - 1].double()
    torch.cuda.synchronize()
    assert rel_l2(out, want) <= KERNEL_GATE
    # layer norm
    x = torch.randn(B, d, generator=g) * 3 + 1
    gam, bet = torch.randn(d, generator=g), torch.randn(d, generator=g)
    y = torch.full((B, d), NAN, device="cuda")
    dev = [t_.cuda() for t_ in (x, gam, bet)]
    _lib.check(lib.ttts_decode_layernorm(*[_p(t_) for t_ in dev], _p(y), B, d, 1e-5, _p(st), s),
               "ttts_decode_layernorm")
    want = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-5)
    torch.cuda.synchronize()
    assert rel_l2(y, want) <= KERNEL_GATE
    # frame out: mel into ys[:, t], stop logits into stop[:, t - 1], the all-stop decision, t advanced
    wm, bm = torch.randn(nm, d, generator=g) / d ** 0.5, torch.randn(nm, generator=g)
    wsp, bsp = torch.randn(1, d, generator=g) / d ** 0.5, torch.tensor([0.1])
    stop = torch.full((B, cap), NAN, device="cuda")
    xo = torch.randn(B, d, generator=g)
    logits = (xo.double() @ wsp.double().T).squeeze(1) + 0.1
    pr = torch.sigmoid(logits)
    dev = [t_.cuda() for t_ in (xo, wm, bm, wsp, bsp)]
    for thr, stops in ((float(pr.min()) - 1e-3, True), (float(pr.min()) + 1e-3, False)):
        st = _state(t, thr=thr)
        _lib.check(lib.ttts_decode_frame_out(*[_p(t_) for t_ in dev], _p(ysd),
                                             cap * nm, _p(stop), cap, B, d, nm, _p(st), s), "ttts_decode_frame_out")
        torch.cuda.synchronize()
        assert rel_l2(ysd[:, t], xo.double() @ wm.double().T + bm.double()) <= KERNEL_GATE
        assert rel_l2(stop[:, t - 1], logits) <= KERNEL_GATE
        assert torch.equal(ysd[:, t + 1:].cpu(), ys[:, t + 1:]) and torch.equal(ysd[:, :t].cpu(), ys[:, :t])
        tv = st.cpu()
        assert int(tv[0]) == t + 1 and int(tv[2]) == (t if stops else -1), (thr, tv)


# ------------------------------------------------------------------------------------------------ the engine
def test_synthesizer_reproduces_the_reference_inference(golden_dir):
    from oracle import oracle_inference
    from transformertts_amd.synthesis import Synthesizer
    g = np.load(os.path.join(golden_dir, "tiny_inference.npz"))
    w_seed = int(g["meta/w_seed"])
    cfg, m = _build(str(g["meta/cfg_name"]), w_seed)
    assert m.emb.weight.shape[1] // m.decoder.layers[0].self_attn.num_heads == 64
    batch, ph, pl = _batch(cfg, int(g["meta/B"]), int(g["meta/Tp"]), int(g["meta/b_seed"]))
    L = int(g["meta/max_len"])
    out = Synthesizer(m)(ph, pl, max_len=L, stop_threshold=2.0)
    fast = m.inference(ph, pl, max_len=L, stop_threshold=2.0, use_kv_cache=True)
    ref = oracle_inference(_oracle64(cfg, w_seed), cfg, batch["phoneme"], batch["phoneme_lens"], max_len=L, stop_threshold=2.0)
    for k in KEYS:
        assert out[k].shape == fast[k].shape == tuple(ref[k].shape) == tuple(g[k].shape), k
        assert out[k].dtype == fast[k].dtype and out[k].device == fast[k].device
        assert rel_l2(out[k], torch.from_numpy(g[k])) < GATE, (k, rel_l2(out[k], torch.from_numpy(g[k])))
        assert rel_l2(out[k], ref[k]) < GATE, (k, rel_l2(out[k], ref[k]))
        assert rel_l2(out[k], fast[k]) < 1e-5, (k, rel_l2(out[k], fast[k]))


@pytest.mark.parametrize("cfg_name,B,Tp,max_len,w_seed,b_seed", [("base", 3, 60, 40, 51, 61), ("scaled", 2, 60, 24, 52, 62),
                                                                 ("micro", 3, 12, 30, 53, 63), ("tiny1h", 3, 12, 30, 54, 64)])
def test_free_running_synthesis_vs_fp64_oracle(cfg_name, B, Tp, max_len, w_seed, b_seed):
    from oracle import oracle_inference
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build(cfg_name, w_seed)
    batch, ph, pl = _batch(cfg, B, Tp, b_seed)
    out = Synthesizer(m)(ph, pl, max_len=max_len, stop_threshold=2.0)
    ref = oracle_inference(_oracle64(cfg, w_seed), cfg, batch["phoneme"], batch["phoneme_lens"], max_len=max_len,
                           stop_threshold=2.0)
    for k in KEYS:
        assert out[k].shape == tuple(ref[k].shape), (k, out[k].shape, ref[k].shape)
        assert rel_l2(out[k], ref[k]) < GATE, (k, rel_l2(out[k], ref[k]))


def test_full_length_frames_are_the_teacher_forced_forward():
    """870 synthesized frames fed back through the eval-mode forward reproduce themselves and the stop logits: every decode
    step at full length, without autoregressive error growth (dense lengths: the masked and unmasked encoders coincide)"""
    from oracle import oracle_forward
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 71)
    batch, ph, pl = _batch(cfg, 4, 100, 72, ragged=False)
    out = Synthesizer(m)(ph, pl, max_len=871, stop_threshold=2.0)
    pred, stop = out["pred_melspec"], out["pred_stop"][..., 0]
    assert pred.shape == (4, 870, cfg["n_mels"]) and stop.shape == (4, 870)
    ml = torch.full((4,), 870, dtype=torch.int64)
    m.eval()
    with torch.no_grad():
        fw = m(ph, pred, pl, ml.cuda(), need_alignments=False)
    assert rel_l2(fw["pred_melspec"], pred) < 1e-5, rel_l2(fw["pred_melspec"], pred)
    assert rel_l2(fw["pred_stop"], stop) < 1e-5, rel_l2(fw["pred_stop"], stop)
    ref = oracle_forward(_oracle64(cfg, 71), cfg, batch["phoneme"], pred.double().cpu(), batch["phoneme_lens"], ml,
                         training=False, dropout=False)
    assert rel_l2(pred, ref["pred_melspec"]) < GATE, rel_l2(pred, ref["pred_melspec"])
    assert rel_l2(stop, ref["pred_stop"]) < GATE, rel_l2(stop, ref["pred_stop"])


def _monotone_stop_head(m, mel, target):
    """make the stop logits of the frames `mel` (B, F, n_mels) follow `target` (F,) for every utterance: the stop head becomes a
    combination of the mel head's rows (its weights do not feed back into the frames, so the frames stay what they were)"""
    wm, bm = m.linear1.linear.weight.detach().double().cpu(), m.linear1.linear.bias.detach().double().cpu()
    A = (mel.double().cpu() - bm).reshape(-1, wm.shape[0])
    a = torch.linalg.pinv(A) @ target.double().repeat(mel.shape[0])
    m.linear2.linear.weight.data.copy_((a @ wm).float().view(1, -1))
    m.linear2.linear.bias.data.zero_()


def test_stop_semantics_and_no_recapture():
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 81)
    _, ph, pl = _batch(cfg, 4, 60, 82)
    synth = Synthesizer(m)
    C = synth.chunk
    L = C + 4                                   # max_len - 1 = C + 3: not a multiple of the chunk
    assert (L - 1) % C != 0
    probe = synth(ph, pl, max_len=L, stop_threshold=2.0)
    assert synth.captures == 1
    F = L - 1
    _monotone_stop_head(m, probe["pred_melspec"], torch.linspace(-3.0, 3.0, F))
    probe = synth(ph, pl, max_len=L, stop_threshold=2.0)           # the engine's own stop probabilities
    p = torch.sigmoid(probe["pred_stop"][..., 0].double()).cpu()   # (B, F)
    low = p.min(dim=0).values
    for f in (C // 2 + 1, C, L - 1):            # inside a chunk, on a chunk boundary, on max_len - 1
        thr = 0.5 * (float(low[:f - 1].max()) + float(low[f - 1]))
        assert float(low[f - 1]) - thr >= 1e-4 and thr - float(low[:f - 1].max()) >= 1e-4, f
        assert float((p[:, :f] - thr).abs().min()) >= 1e-4, f
        out = synth(ph, pl, max_len=L, stop_threshold=thr)
        ref = m.inference(ph, pl, max_len=L, stop_threshold=thr)
        assert out["pred_melspec"].shape[1] == f == ref["pred_melspec"].shape[1], (f, out["pred_melspec"].shape)
        for k in KEYS:
            assert out[k].shape == ref[k].shape and rel_l2(out[k], ref[k]) < 1e-5, (f, k, rel_l2(out[k], ref[k]))
    one = synth(ph, pl, max_len=L, stop_threshold=0.0)
    assert one["pred_melspec"].shape[1] == 1 and one["pred_stop"].shape == (4, 1, 1)
    short = synth(ph, pl, max_len=7, stop_threshold=2.0)
    assert short["pred_melspec"].shape[1] == 6
    assert torch.equal(short["pred_melspec"], probe["pred_melspec"][:, :6])
    assert synth.captures == 1                  # max_len and the threshold changed, nothing was captured again


def test_eager_first_call_and_replays_are_bitwise_equal_and_eviction_recaptures():
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 91)
    _, ph, pl = _batch(cfg, 3, 50, 92)
    synth = Synthesizer(m)
    L = 2 * synth.chunk + 5
    runs = [synth(ph, pl, max_len=L, stop_threshold=2.0) for _ in range(3)]
    assert synth.captures == 1
    for r in runs[1:]:
        for k in KEYS:
            assert torch.equal(r[k], runs[0][k]), k
    shapes = [_batch(cfg, 1, 30, 93)[1:], _batch(cfg, 2, 70, 94)[1:], _batch(cfg, 3, 130, 95)[1:]]
    small = Synthesizer(m, max_shapes=2)
    first = [small(p_, l_, max_len=20, stop_threshold=2.0) for p_, l_ in shapes]
    again = [small(p_, l_, max_len=20, stop_threshold=2.0) for p_, l_ in shapes]
    assert small.captures == 6 and len(small.shape_bytes()) == 2
    for a, b in zip(first, again):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k


def test_weights_are_followed():
    from oracle import fill_state
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 101)
    _, ph, pl = _batch(cfg, 2, 40, 102)
    synth = Synthesizer(m)
    a = synth(ph, pl, max_len=20, stop_threshold=2.0)
    m.load_state_dict(fill_state(cfg, 103), strict=True)            # in place
    b = synth(ph, pl, max_len=20, stop_threshold=2.0)
    fresh = Synthesizer(m)(ph, pl, max_len=20, stop_threshold=2.0)
    assert synth.captures == 1 and not torch.equal(a["pred_melspec"], b["pred_melspec"])
    for k in KEYS:
        assert torch.equal(b[k], fresh[k]), k
    lin = m.decoder.layers[1].linear1
    lin.weight = torch.nn.Parameter(lin.weight.detach() * 1.25)     # a new parameter object: new storage
    c = synth(ph, pl, max_len=20, stop_threshold=2.0)
    fresh = Synthesizer(m)(ph, pl, max_len=20, stop_threshold=2.0)
    assert synth.captures == 2 and synth.recaptures == 1
    assert not torch.equal(c["pred_melspec"], b["pred_melspec"])
    for k in KEYS:
        assert torch.equal(c[k], fresh[k]), k


def test_an_utterance_does_not_depend_on_its_batch():
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("base", 111)
    _, ph, pl = _batch(cfg, 5, 80, 112)
    synth = Synthesizer(m)
    full = synth(ph, pl, max_len=33, stop_threshold=2.0)
    for i in (0, 3):
        alone = synth(ph[i:i + 1], pl[i:i + 1], max_len=33, stop_threshold=2.0)
        for k in KEYS:
            assert alone[k].shape[1] == 32 and rel_l2(alone[k], full[k][i:i + 1]) < 1e-5, (i, k, rel_l2(alone[k], full[k][i:i + 1]))
