"""Phoneme durations from the alignment maps (csrc/alignment.hip; transformertts_amd/alignment.py): focus rate and row argmax
against fp64 torch, the head choice, argmax durations against `bincount`, the monotonic alignment search against planted paths
and an fp64 dynamic programme, what is (not) read past the lengths, strided maps, graph capture, and the two callers
(`teacher_durations` on the teacher-forced forward, `extract_durations` on the synthesizer's maps).

L = 2, B = 5, H = 4, Tm = 150; Tp = 13 (no multiple of 4, one phoneme per lane), 70 (crosses the 64-lane boundary: two per lane)
and 130 (three 64-column groups: four per lane).  Lengths: (T, N) = (Tm, Tp); T = N (the search is forced onto the diagonal); N = 1;
T = N = 1; T < N (no path: valid is False, the row zero)."""
import functools
import math
import os

import pytest
import torch

from conftest import rel_l2
from test_hip_dropout_parity import REPORT_DIR
from test_hip_model import _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, H, TM = 2, 5, 4, 150
TPS = (13, 70, 130)
TINY = torch.tensor(1e-30, dtype=torch.float32).double()       # the kernel's floor under the logarithm, as fp32 holds it


def _lens(Tp):
    plens = torch.tensor([Tp, Tp - 2, 1, 1, 9])
    mlens = torch.tensor([TM, Tp - 2, 37, 1, 5])
    return plens, mlens


def _random_maps(Tp, seed):
    """row-stochastic over the live columns; rows and columns past the lengths hold zeros"""
    plens, mlens = _lens(Tp)
    g = torch.Generator().manual_seed(seed)
    live = (torch.arange(Tp)[None, :] < plens[:, None])[:, None, None, :]
    rows = (torch.arange(TM)[None, :] < mlens[:, None])[:, None, :, None]
    out = []
    for _ in range(L):
        a = torch.rand(B, H, TM, Tp, generator=g) ** 4 * live                 # (peaky rows: focus rates away from 1 / N)
        out.append((a / a.sum(-1, keepdim=True).clamp_min(1e-30) * rows).float())
    return out


def _tie_columns(Tp):
    """(first, second) columns of planted equal maxima: the same lane of two 64-column groups, and a later column in a LOWER lane"""
    return [(4, 11), (2, 9)] if Tp == 13 else [(3, 67), (10, 65)]


@functools.lru_cache(maxsize=None)
def _case(Tp):
    """-> (maps on the CPU, plens, mlens, oracle argmax (L,B,H,Tm) int64 with 0 past T_b, oracle focus (L,B,H) fp64)"""
    plens, mlens = _lens(Tp)
    maps = _random_maps(Tp, 100 + Tp)
    (a1, a2), (b1, b2) = _tie_columns(Tp)
    maps[0][0, :, 5:40:3, a1] = 2.0                                           # two equal maxima per row, utterance 0 (N = Tp)
    maps[0][0, :, 5:40:3, a2] = 2.0
    maps[1][0, :, 7:50:5, b1] = 3.0
    maps[1][0, :, 7:50:5, b2] = 3.0
    amax = torch.zeros(L, B, H, TM, dtype=torch.int64)
    focus = torch.zeros(L, B, H, dtype=torch.float64)
    for l, m in enumerate(maps):
        for b in range(B):
            T, N = int(mlens[b]), int(plens[b])
            sub = m[b, :, :T, :N].double()
            amax[l, b, :, :T] = torch.argmax(sub, -1)
            focus[l, b] = sub.max(-1).values.sum(-1) / T
    return maps, plens, mlens, amax, focus


def _extract(maps, plens, mlens, **kw):
    from transformertts_amd.alignment import extract_durations
    out = extract_durations([m.to(DEV) for m in maps], plens.to(DEV), mlens.to(DEV), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _mas64(A, T, N):
    """the search restated in fp64 as a loop over t, vectorised over n -> (durations (N,), Q*); A: (Tm, Tp) fp32"""
    s = torch.log(torch.maximum(A[:T, :N].double(), TINY))
    n = torch.arange(N)
    neg = torch.tensor([-math.inf], dtype=torch.float64)
    q = torch.full((N,), -math.inf, dtype=torch.float64)
    q[0] = s[0, 0]
    stays = torch.ones(T, N, dtype=torch.bool)
    for t in range(1, T):
        adv = torch.cat([neg, q[:-1]])
        stay = q >= adv
        stays[t] = stay
        inside = (n <= t) & (N - 1 - n <= T - 1 - t)
        q = torch.where(inside, s[t] + torch.where(stay, q, adv), neg)
    dur = torch.zeros(N, dtype=torch.int64)
    k = N - 1
    for t in range(T - 1, -1, -1):
        dur[k] += 1
        if t > 0 and not stays[t, k]:
            k -= 1
    assert k == 0
    return dur, float(q[N - 1])


def _path_score64(A, dur, T, N):
    """fp64 score of the monotonic path that spends dur[n] frames on phoneme n"""
    path = torch.repeat_interleave(torch.arange(N), dur[:N])
    assert path.numel() == T
    return float(torch.log(torch.maximum(A[torch.arange(T), path].double(), TINY)).sum())


# ================================================================================================ 1. focus rate and argmax
@pytest.mark.parametrize("Tp", TPS)
def test_focus_rate_and_row_argmax_vs_fp64(Tp):
    from transformertts_amd.alignment import _operands, _rowstats
    maps, plens, mlens, amax64, focus64 = _case(Tp)
    dmaps, strides = _operands([m.to(DEV) for m in maps])
    amax, focus = _rowstats(dmaps, strides, plens.to(DEV), mlens.to(DEV))
    torch.cuda.synchronize()
    assert amax.dtype == torch.int32 and tuple(amax.shape) == (L, B, H, TM) and tuple(focus.shape) == (L, B, H)
    assert torch.equal(amax.cpu().long(), amax64)                             # exactly torch.argmax, 0 past T_b
    (a1, a2), (b1, b2) = _tie_columns(Tp)
    assert bool((amax64[0, 0, :, 5:40:3] == a1).all()) and bool((amax64[1, 0, :, 7:50:5] == b1).all())    # the ties are there
    err = ((focus.cpu().double() - focus64).abs() / focus64.abs()).max().item()
    print(f"focus rate Tp={Tp}: worst relative error {err:.3e} (gate 1e-5)")
    assert err < 1e-5
    out = _extract(maps, plens, mlens, method="argmax")
    assert torch.equal(out["focus_rate"], focus.cpu())


def test_focus_rate_is_zero_without_frames_or_phonemes():
    maps, plens, mlens, _, _ = _case(13)
    plens, mlens = plens.clone(), mlens.clone()
    plens[1], mlens[2] = 0, 0
    for method in ("argmax", "mas"):
        out = _extract(maps, plens, mlens, method=method)
        assert float(out["focus_rate"][:, 1].abs().sum()) == 0.0 and float(out["focus_rate"][:, 2].abs().sum()) == 0.0
        assert out["valid"].tolist() == [True, False, False, True, False if method == "mas" else True]
        assert int(out["durations"][1].abs().sum()) == 0 and int(out["durations"][2].abs().sum()) == 0
    # lengths beyond the maps are clamped to them
    big = _extract(maps, plens + 1000 * (plens > 1), mlens + 1000 * (mlens > 100), method="mas")
    ref = _extract(maps, torch.where(plens > 1, torch.tensor(13), plens), torch.where(mlens > 100, torch.tensor(TM), mlens), method="mas")
    for k in ref:
        assert torch.equal(big[k], ref[k]), k


# ================================================================================================ 2. head choice
def _first_max(F):
    """F (L, B, H) -> per b the first maximum over layer * H + head, as (layer, head) rows"""
    c = F.permute(1, 0, 2).reshape(F.shape[1], -1).argmax(-1)
    return torch.stack([c // F.shape[2], c % F.shape[2]], -1)


def _batch_choice(F, plens, mlens):
    tot = torch.zeros(F.shape[0], F.shape[2], dtype=torch.float32)
    for b in range(F.shape[1]):                                               # fp32, in b order, as the kernel adds
        if plens[b] > 0 and mlens[b] > 0:
            tot = tot + F[:, b]
    c = int(tot.reshape(-1).argmax())
    return torch.tensor([[c // F.shape[2], c % F.shape[2]]] * F.shape[1])


@pytest.mark.parametrize("Tp", TPS)
def test_head_choice_is_the_first_maximum_of_the_kernels_focus_rate(Tp):
    maps, plens, mlens, _, _ = _case(Tp)
    utt = _extract(maps, plens, mlens, method="argmax", select="utterance")
    F = utt["focus_rate"]
    assert utt["choice"].dtype == torch.int64 and torch.equal(utt["choice"], _first_max(F))
    assert len({tuple(r) for r in utt["choice"].tolist()}) > 1                # (the utterances do not all agree)
    bat = _extract(maps, plens, mlens, method="argmax", select="batch")
    assert torch.equal(bat["choice"], _batch_choice(F, plens, mlens)) and torch.equal(bat["focus_rate"], F)
    fix = _extract(maps, plens, mlens, method="argmax", select=(1, 2))
    assert torch.equal(fix["choice"], torch.tensor([[1, 2]] * B))
    # an utterance without frames does not count in the batch's sum
    p0, m0 = plens.clone(), mlens.clone()
    m0[0] = 0
    bat0 = _extract(maps, p0, m0, method="argmax", select="batch")
    assert torch.equal(bat0["choice"], _batch_choice(bat0["focus_rate"], p0, m0))


def test_head_choice_of_two_bit_identical_heads_is_the_lower_index():
    maps, plens, mlens, _, _ = _case(70)
    maps = [m.clone() for m in maps]
    sharp = torch.zeros(B, TM, 70)                                            # (not row-stochastic: above every random head)
    sharp[:, torch.arange(TM), (torch.arange(TM) * 7) % 9] = 5.0              # peaks in columns < 9 <= every N_b > 1 ...
    sharp[:, :, 0] += 1.5                                                     # ... and N_b = 1 reads column 0 alone
    maps[0][:, 1] = sharp
    maps[1][:, 3] = sharp
    maps[1][:, 0] = sharp
    for select in ("utterance", "batch"):
        out = _extract(maps, plens, mlens, method="argmax", select=select)
        F = out["focus_rate"]
        assert torch.equal(F[0, :, 1], F[1, :, 3]) and torch.equal(F[0, :, 1], F[1, :, 0])
        assert torch.equal(out["choice"], torch.tensor([[0, 1]] * B)), (select, out["choice"])


# ================================================================================================ 3. argmax durations
@pytest.mark.parametrize("Tp", TPS)
@pytest.mark.parametrize("select", ["utterance", "batch", (0, 3)])
def test_argmax_durations_equal_bincount(Tp, select):
    maps, plens, mlens, amax64, _ = _case(Tp)
    out = _extract(maps, plens, mlens, method="argmax", select=select)
    dur = out["durations"]
    assert dur.dtype == torch.int64 and tuple(dur.shape) == (B, Tp) and out["valid"].dtype == torch.bool and bool(out["valid"].all())
    for b in range(B):
        T, N = int(mlens[b]), int(plens[b])
        l, h = out["choice"][b].tolist()
        assert torch.equal(dur[b], torch.bincount(amax64[l, b, h, :T], minlength=Tp)), b
        assert int(dur[b].sum()) == T and int(dur[b, N:].abs().sum()) == 0


# ================================================================================================ 4. MAS, planted paths
def _planted(Tp, seed):
    """maps that carry 0.9 on a random monotonic path per (layer, b, h) and the rest spread evenly -> (maps, durations (L,B,H,Tp))"""
    plens, mlens = _lens(Tp)
    g = torch.Generator().manual_seed(seed)
    maps = _random_maps(Tp, seed)
    durs = torch.zeros(L, B, H, Tp, dtype=torch.int64)
    for l in range(L):
        for b in range(B):
            T, N = int(mlens[b]), int(plens[b])
            if T < N:
                continue
            for h in range(H):
                cuts = (torch.randperm(T - 1, generator=g)[:N - 1] + 1).sort().values
                edges = torch.cat([torch.tensor([0]), cuts, torch.tensor([T])])
                d = edges[1:] - edges[:-1]
                path = torch.repeat_interleave(torch.arange(N), d)
                a = torch.full((T, N), 0.1 / max(N - 1, 1))
                a[torch.arange(T), path] = 0.9 if N > 1 else 1.0
                maps[l][b, h, :T, :N] = a
                durs[l, b, h, :N] = d
    return maps, durs


@pytest.mark.parametrize("Tp", TPS)
def test_mas_recovers_planted_paths(Tp):
    plens, mlens = _lens(Tp)
    maps, planted = _planted(Tp, 300 + Tp)
    for l, h in ((0, 0), (1, 2)):
        out = _extract(maps, plens, mlens, method="mas", select=(l, h))
        assert out["valid"].tolist() == [True, True, True, True, False]
        assert torch.equal(out["choice"], torch.tensor([[l, h]] * B))
        for b in range(B):
            T, N = int(mlens[b]), int(plens[b])
            if T < N:
                assert int(out["durations"][b].abs().sum()) == 0              # no path: the row is zero
                continue
            assert torch.equal(out["durations"][b], planted[l, b, h]), (l, h, b)
            assert torch.equal(out["durations"][b, :N], _mas64(maps[l][b, h], T, N)[0]), (l, h, b)
        assert bool((out["durations"][1, :int(plens[1])] == 1).all())         # T = N: the diagonal
        assert int(out["durations"][2, 0]) == int(mlens[2]) and int(out["durations"][3, 0]) == 1       # N = 1


# ================================================================================================ 5. MAS, random maps
def test_mas_on_random_maps_is_monotonic_and_optimal_within_fp32():
    """every valid row: durations >= 1 for n < N_b that sum to T_b (so the path is monotonic and visits every phoneme), and its
    fp64 score is within 8 T_b 2^-24 |Q*| of the fp64 optimum Q*: T_b fp32 additions that each round by at most 2^-24 |Q|, twice
    (two paths are compared), and twice again for logf.  Worst measured gap / bound: alignment_mas_gap.txt in REPORT_DIR
    (as measured on one MI355X: tests/reports/alignment_mas_gap.txt)."""
    lines, worst = [], 0.0
    for Tp in TPS:
        maps, plens, mlens, _, _ = _case(Tp)
        for select in ("utterance", (0, 1), (1, 3)):
            out = _extract(maps, plens, mlens, method="mas", select=select)
            assert out["valid"].tolist() == [True, True, True, True, False]
            for b in range(B):
                T, N = int(mlens[b]), int(plens[b])
                d = out["durations"][b]
                if T < N:
                    assert int(d.abs().sum()) == 0
                    continue
                assert int(d[:N].min()) >= 1 and int(d.sum()) == T and int(d[N:].abs().sum()) == 0
                l, h = out["choice"][b].tolist()
                _, q_star = _mas64(maps[l][b, h], T, N)
                gap = q_star - _path_score64(maps[l][b, h], d, T, N)
                bound = 8 * T * 2.0 ** -24 * abs(q_star)
                ratio = gap / bound if bound > 0 else 0.0
                lines.append(f"Tp={Tp} select={select} b={b} T={T} N={N} Q*={q_star:.6f} gap={gap:.3e} bound={bound:.3e} ratio={ratio:.3e}")
                print(lines[-1])
                worst = max(worst, ratio)
                assert -1e-9 * abs(q_star) <= gap <= bound, lines[-1]           # (below zero: the two fp64 sums' own rounding)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/alignment_mas_gap.txt", "w") as f:
        f.write("\n".join(lines) + f"\nworst gap / bound: {worst:.3e}\n")


# ================================================================================================ 6. nothing past the lengths
@pytest.mark.parametrize("Tp", TPS)
def test_nothing_past_the_lengths_is_read(Tp):
    maps, plens, mlens, _, _ = _case(Tp)
    dead = ~((torch.arange(TM)[None, :, None] < mlens[:, None, None]) & (torch.arange(Tp)[None, None, :] < plens[:, None, None]))
    poison = torch.where((torch.arange(TM)[:, None] + torch.arange(Tp)[None, :]) % 2 == 0, torch.tensor(float("nan")), torch.tensor(1e30))
    dirty = [torch.where(dead[:, None], poison, m) for m in maps]
    assert all(bool(torch.isnan(d).any()) for d in dirty)
    for method in ("mas", "argmax"):
        for select in ("utterance", "batch"):
            clean, got = _extract(maps, plens, mlens, method=method, select=select), _extract(dirty, plens, mlens, method=method, select=select)
            assert set(got) == {"durations", "focus_rate", "choice", "valid"}
            for k in clean:
                assert torch.equal(clean[k], got[k]), (method, select, k)


# ================================================================================================ 7. strided maps
@pytest.mark.parametrize("Tp", TPS)
def test_strided_maps_are_read_in_place(Tp):
    from transformertts_amd.alignment import _operands, extract_durations
    maps, plens, mlens, _, _ = _case(Tp)
    ld = (Tp + 3 + 3) // 4 * 4
    views = []
    for m in maps:
        buf = torch.full((B, H, TM, ld), float("nan"), device=DEV)
        buf[..., :Tp] = m.to(DEV)
        views.append(buf[..., :Tp])
    used, strides = _operands(views)
    assert strides == (ld, TM * ld, H * TM * ld)
    assert [u.data_ptr() for u in used] == [v.data_ptr() for v in views] and all(not v.is_contiguous() for v in views)     # no copy
    for method in ("mas", "argmax"):
        got = extract_durations(views, plens.to(DEV), mlens.to(DEV), method=method)
        ref = _extract(maps, plens, mlens, method=method)
        for k in ref:
            assert torch.equal(got[k].cpu(), ref[k]), (method, k)
    # a layout the kernels cannot address is copied once and gives the same result
    t = [m.to(DEV).transpose(2, 3).contiguous().transpose(2, 3) for m in maps]
    assert _operands(t)[0][0].data_ptr() != t[0].data_ptr()
    got = extract_durations(t, plens.to(DEV), mlens.to(DEV))
    for k, v in _extract(maps, plens, mlens).items():
        assert torch.equal(got[k].cpu(), v), k


# ================================================================================================ 8. graph capture
def test_both_methods_capture_into_one_graph_and_replay_bitwise():
    from transformertts_amd.alignment import extract_durations
    Tp = 70
    plens, mlens = _lens(Tp)
    dp, dm = plens.to(DEV), mlens.to(DEV)
    static = [m.to(DEV) for m in _random_maps(Tp, 1)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                             # (warm-up: the library is loaded, the allocator primed)
        extract_durations(static, dp, dm, method="mas")
        extract_durations(static, dp, dm, method="argmax", select="batch")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_mas = extract_durations(static, dp, dm, method="mas")
        g_arg = extract_durations(static, dp, dm, method="argmax", select="batch")
    seen = []
    for seed in (2, 3):
        fresh = _planted(Tp, seed)[0] if seed == 3 else _random_maps(Tp, seed)
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        for got, kw in ((g_mas, dict(method="mas")), (g_arg, dict(method="argmax", select="batch"))):
            ref = _extract(fresh, plens, mlens, **kw)
            for k in ref:
                assert torch.equal(got[k].cpu(), ref[k]), (seed, kw, k)
        seen.append(g_mas["durations"].cpu().clone())
    assert not torch.equal(seen[0], seen[1])                                  # the replays did follow the maps


# ================================================================================================ 9. end to end
@pytest.mark.parametrize("training", [True, False])
def test_teacher_durations_on_the_tiny_model(training):
    from oracle import synth_batch
    from transformertts_amd import teacher_durations
    cfg, m = _build("tiny", 11)
    m.train(training)
    next(iter(m.children())).eval()                                           # a model of mixed modes keeps every module's own flag
    flags = [mod.training for mod in m.modules()]
    assert (len(set(flags)) == 2) is training
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    args = [batch[k].to(DEV) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    for method in ("mas", "argmax"):
        out = teacher_durations(m, *args, method=method)
        torch.cuda.synchronize()
        assert m.training is training and [mod.training for mod in m.modules()] == flags
        assert set(out) == {"durations", "focus_rate", "choice", "valid", "pred_melspec"}
        assert tuple(out["durations"].shape) == (3, 12) and out["durations"].dtype == torch.int64
        assert tuple(out["pred_melspec"].shape) == tuple(batch["melspec"].shape)
        valid = out["valid"].cpu()
        assert bool(valid.any()) and valid.tolist() == (batch["melspec_lens"] >= batch["phoneme_lens"]).tolist()
        assert torch.equal(out["durations"].sum(-1).cpu()[valid], batch["melspec_lens"][valid])
        if method == "mas":
            for b in range(3):
                assert int(out["durations"][b, :int(batch["phoneme_lens"][b])].min()) >= 1
    m.eval()
    with torch.no_grad():
        ref = m(*args, need_alignments=True)
    assert rel_l2(out["pred_melspec"], ref["pred_melspec"]) < 1e-6            # the eval-mode forward, whatever mode the model was in


def test_durations_from_the_synthesizers_maps():
    from oracle import synth_batch
    from transformertts_amd import extract_durations
    from transformertts_amd.synthesis import Synthesizer
    cfg, m = _build("tiny", 11)
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=21)
    ph, pl = batch["phoneme"].to(DEV), batch["phoneme_lens"].to(DEV)
    out = Synthesizer(m).synthesize(ph, pl, max_len=24, stop_threshold=2.0, alignments=True)
    for method in ("mas", "argmax"):
        res = extract_durations(out["alignments"], pl, out["mel_lens"], method=method)
        torch.cuda.synchronize()
        assert tuple(res["durations"].shape) == (3, 12) and bool(res["valid"].all())
        assert torch.equal(res["durations"].sum(-1), out["mel_lens"])
        assert tuple(res["focus_rate"].shape) == (len(out["alignments"]), 3, out["alignments"][0].shape[1])
