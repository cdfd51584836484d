#!/usr/bin/env python3
"""What reading phoneme durations off the alignment maps costs: `extract_durations` (csrc/alignment.hip) against
the same extraction restated in stock torch on the same device, alternating round by round in one process.

    python tools/durations_bench.py [--batch 64] [--rounds 5] [--reps 10] [--torch-reps 2]

Base shape: L = 3 decoder layers, B = 64, the base model's head count, Tm = 870, Tp = 160, ragged lengths, select="utterance".
The stock-torch restatement: per map `max(-1)` (values and argmax), a masked mean for the focus rate, the head picked by an
`argmax` and an indexed gather on the device, then
    argmax   one `torch.bincount` per utterance (the lengths are known on the host, as in a data-preparation script);
    mas      the dynamic programme as a Python loop over the frames, vectorised over (B, Tp), and its backtrack likewise.
Prints one JSON line per method (times in microseconds per call, device events around `reps` calls); `equal_rows` counts the
utterances whose durations agree with the kernels' (argmax: all of them, exactly; mas: both run in fp32 with different
logarithms, so a near-tie may fall differently)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def make_case(L, B, H, Tm, Tp, device, seed=1234):
    """peaky row-stochastic maps with zeros past the ragged lengths; utterance 0 has the full extent"""
    g = torch.Generator().manual_seed(seed)
    plens = torch.randint(Tp * 3 // 8, Tp + 1, (B,), generator=g)
    mlens = torch.maximum(torch.randint(Tm // 2, Tm + 1, (B,), generator=g), plens)
    plens[0], mlens[0] = Tp, Tm
    dp, dm = plens.to(device), mlens.to(device)
    live = (torch.arange(Tp, device=device)[None, :] < dp[:, None])[:, None, None, :]
    rows = (torch.arange(Tm, device=device)[None, :] < dm[:, None])[:, None, :, None]
    torch.manual_seed(seed)
    maps = []
    for _ in range(L):
        a = torch.rand(B, H, Tm, Tp, device=device) ** 4 * live
        maps.append(a / a.sum(-1, keepdim=True).clamp_min(1e-30) * rows)
    return maps, plens, mlens


def torch_stats(maps, dp, dm):
    """-> (focus (L,B,H), chosen plane's row argmax (B,Tm), choice (B,) = layer * H + head)"""
    B, H, Tm, Tp = maps[0].shape
    rows = (torch.arange(Tm, device=dp.device)[None, :] < dm[:, None])[:, None, :]
    mx, am = zip(*(m.max(-1) for m in maps))
    focus = torch.stack([(v * rows).sum(-1) / dm.clamp_min(1)[:, None] for v in mx])
    choice = focus.permute(1, 0, 2).reshape(B, -1).argmax(-1)
    return focus, pick_plane(am, choice, H), choice


def pick_plane(per_layer, choice, H):
    """per_layer: L tensors (B, H, ...) -> (B, ...), utterance b taking head choice[b] % H of layer choice[b] // H; one gather per
    layer and a select, so that no copy of all L tensors is made"""
    b = torch.arange(choice.shape[0], device=choice.device)
    out = per_layer[0][b, choice % H]
    for l in range(1, len(per_layer)):
        mine = (choice // H == l).reshape(-1, *([1] * (out.dim() - 1)))
        out = torch.where(mine, per_layer[l][b, choice % H], out)
    return out


def torch_argmax(maps, dp, dm, plens, mlens):
    focus, am, choice = torch_stats(maps, dp, dm)
    Tp = maps[0].shape[-1]
    dur = torch.stack([torch.bincount(am[b, :int(mlens[b])], minlength=Tp) for b in range(len(plens))])
    return dur, focus, choice


def torch_mas(maps, dp, dm, plens, mlens):
    focus, _, choice = torch_stats(maps, dp, dm)
    B, H, Tm, Tp = maps[0].shape
    dev = dp.device
    s = torch.log(pick_plane(maps, choice, H).clamp_min(1e-30))                           # (B, Tm, Tp)
    n = torch.arange(Tp, device=dev)[None, :]
    T, N = dm[:, None], dp[:, None]
    neg = torch.full((B, 1), -math.inf, device=dev)
    q = torch.full((B, Tp), -math.inf, device=dev)
    q[:, 0] = s[:, 0, 0]
    stays = torch.ones(Tm, B, Tp, dtype=torch.bool, device=dev)
    for t in range(1, Tm):
        adv = torch.cat([neg, q[:, :-1]], 1)
        stay = q >= adv
        stays[t] = stay
        inside = (n <= t) & (N - 1 - n <= T - 1 - t) & (n < N)
        q = torch.where(T > t, torch.where(inside, s[:, t] + torch.where(stay, q, adv), neg), q)
    dur = torch.zeros(B, Tp, dtype=torch.int64, device=dev)
    k = (dp - 1).clamp_min(0)
    for t in range(Tm - 1, -1, -1):
        on = dm > t
        dur.scatter_add_(1, k[:, None], on.long()[:, None])
        if t > 0:
            k = k - (on & ~stays[t].gather(1, k[:, None])[:, 0]).long()
    return dur * (dm >= dp)[:, None], focus, choice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    a = ap.parse_args()
    from transformertts_amd import extract_durations
    from transformertts_amd.workload import model_config
    if not torch.cuda.is_available():
        raise SystemExit("durations_bench: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    L, B, H, Tm, Tp = 3, a.batch, model_config("base")["decoder_n_head"], 870, 160
    maps, plens, mlens = make_case(L, B, H, Tm, Tp, dev)
    dp, dm = plens.to(dev), mlens.to(dev)
    stock = {"argmax": torch_argmax, "mas": torch_mas}
    for method in ("argmax", "mas"):
        ours = lambda: extract_durations(maps, dp, dm, method=method, select="utterance")
        theirs = lambda: stock[method](maps, dp, dm, plens, mlens)
        got, ref = ours(), theirs()                                               # (warm-up, and the comparison)
        torch.cuda.synchronize()
        equal = int((got["durations"] == ref[0]).all(-1).sum())
        same_choice = bool(torch.equal(got["choice"][:, 0] * H + got["choice"][:, 1], ref[2]))
        focus_err = float(((got["focus_rate"] - ref[1]).abs() / ref[1].abs().clamp_min(1e-30)).max())
        t_ours, t_theirs = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours, a.reps))
            t_theirs.append(timed(theirs, a.torch_reps if method == "mas" else a.reps))
        print(json.dumps({
            "tool": "durations_bench", "method": method, "select": "utterance",
            "shape": {"L": L, "B": B, "H": H, "Tm": Tm, "Tp": Tp, "mean_T": float(mlens.float().mean()), "mean_N": float(plens.float().mean())},
            "map_bytes": L * B * H * Tm * Tp * 4, "rounds": a.rounds, "reps": a.reps,
            "kernels_us": {"min": round(min(t_ours), 1), "median": round(statistics.median(t_ours), 1)},
            "stock_torch_us": {"min": round(min(t_theirs), 1), "median": round(statistics.median(t_theirs), 1)},
            "stock_over_kernels": round(statistics.median(t_theirs) / statistics.median(t_ours), 2),
            "equal_rows": equal, "rows": B, "same_choice": same_choice, "focus_rate_max_rel_diff": focus_err}), flush=True)


if __name__ == "__main__":
    main()
