#!/usr/bin/env python3
"""What the DTW mel distance costs: `dtw_distance` (csrc/dtw.hip) against the same computation restated in stock
torch on the same device, alternating round by round in one process.

    python tools/dtw_bench.py [--rounds 5] [--reps 20] [--torch-reps 1]

Configurations, C = 80 mel bins, metric l1: B = 1 and B = 16 at 870 x 870 frames, and B = 16 ragged with lengths 300 .. 1499 on
both sides.  The stock-torch restatement (`torch_dtw`, nothing taken from outside this file): the cells as C elementwise passes in
channel order (the kernels' order, so the two sides agree bit for bit; a batched `torch.cdist` of this size did not give usable
values on the device), one gather that lays the anti-diagonals out as rows, a Python loop over the Tx + Ty - 1 anti-diagonals
vectorised over (B, Tx) that keeps the 2-bit directions, and a Python loop for the backtrack, every step on the device (no host
read inside either loop).  Prints one JSON line per configuration (times in microseconds per call, device events around `reps`
calls; medians and minima over the rounds); `equal_cost` and `equal_path_len` count the utterances on which the two sides agree
exactly, `cost_max_rel_diff` is the largest relative difference of the costs."""
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


def make_case(B, Tx, Ty, C, device, ragged=None, seed=1234):
    """standard-normal features; `ragged` = (lo, hi): lengths drawn from lo .. hi on both sides, utterance 0 at the full extent"""
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(B, Tx, C, generator=g), torch.randn(B, Ty, C, generator=g)
    xl, yl = torch.full((B,), Tx), torch.full((B,), Ty)
    if ragged is not None:
        xl = torch.randint(ragged[0], ragged[1] + 1, (B,), generator=g).clamp(max=Tx)
        yl = torch.randint(ragged[0], ragged[1] + 1, (B,), generator=g).clamp(max=Ty)
        xl[0], yl[0] = Tx, Ty
    return x.to(device), xl.to(device), y.to(device), yl.to(device)


def torch_dtw(x, xl, y, yl, metric="l1"):
    """-> (cost (B,) fp32, path_len (B,) int64); the recurrence, the tie rule (diagonal, then (i-1, j), then (i, j-1)) and the
    clamped lengths of csrc/dtw.hip; zero for a row with a zero length"""
    B, Tx, _ = x.shape
    Ty, dev = y.shape[1], x.device
    n, m = xl.clamp(0, Tx), yl.clamp(0, Ty)
    c = torch.zeros(B, Tx, Ty, device=dev)
    for k in range(x.shape[2]):
        diff = x[:, :, None, k] - y[:, None, :, k]
        c = c + (diff.abs() if metric == "l1" else diff * diff)
    c = c if metric == "l1" else c.sqrt()
    i = torch.arange(Tx, device=dev)
    D = Tx + Ty - 1
    j = torch.arange(D, device=dev)[:, None] - i[None, :]                                 # (D, Tx): the column of row i on diagonal d
    skew = c.gather(2, j.clamp(0, Ty - 1).T[None].expand(B, Tx, D)).permute(2, 0, 1)      # (D, B, Tx)
    inf = torch.full((B, 1), math.inf, device=dev)
    on_all = (j >= 0)[:, None, :] & (j[:, None, :] < m[None, :, None]) & (i[None, None, :] < n[None, :, None])   # (D, B, Tx)
    prev2 = torch.full((B, Tx), math.inf, device=dev)
    prev1 = torch.where(on_all[0], skew[0], prev2)                                        # D[0][0] = c[0][0]
    steps = torch.zeros(D, B, Tx, dtype=torch.int8, device=dev)
    last = n + m - 2
    cost = torch.where(last == 0, prev1[:, 0], torch.zeros(B, device=dev))
    rows = (n - 1).clamp(min=0)[:, None]
    for d in range(1, D):
        diag = torch.cat([inf, prev2[:, :-1]], 1)
        up = torch.cat([inf, prev1[:, :-1]], 1)
        best = torch.minimum(torch.minimum(diag, up), prev1)
        steps[d] = torch.where(diag == best, 0, torch.where(up == best, 1, 2))
        prev2, prev1 = prev1, torch.where(on_all[d], skew[d] + best, math.inf)
        cost = torch.where(last == d, prev1.gather(1, rows)[:, 0], cost)
    valid = (n > 0) & (m > 0)
    pi, pj = (n - 1).clamp(min=0), (m - 1).clamp(min=0)
    plen = valid.long()
    b = torch.arange(B, device=dev)
    for _ in range(D - 1):
        s = steps[pi + pj, b, pi]
        s = torch.where(pi == 0, 2, torch.where(pj == 0, 1, s.long()))
        go = valid & ((pi > 0) | (pj > 0))
        pi, pj = pi - (go & (s != 2)).long(), pj - (go & (s != 1)).long()
        plen = plen + go.long()
    return torch.where(valid, cost, torch.zeros_like(cost)), plen


CONFIGS = (("B1_870x870", 1, 870, 870, None), ("B16_870x870", 16, 870, 870, None), ("B16_ragged_300_1499", 16, 1499, 1499, (300, 1499)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=1)
    a = ap.parse_args()
    from transformertts_amd import dtw_distance
    if not torch.cuda.is_available():
        raise SystemExit("dtw_bench: needs the GPU (a CPU timing says nothing about it)")
    dev, C = torch.device("cuda:0"), 80
    for name, B, Tx, Ty, ragged in CONFIGS:
        x, xl, y, yl = make_case(B, Tx, Ty, C, dev, ragged)
        ours = lambda: dtw_distance(x, xl, y, yl, metric="l1")
        theirs = lambda: torch_dtw(x, xl, y, yl, "l1")
        got, ref = ours(), theirs()                                                       # (warm-up, and the comparison)
        torch.cuda.synchronize()
        rel = float(((got["cost"] - ref[0]).abs() / ref[0].abs().clamp_min(1e-30)).max())
        same_len, same_cost = int((got["path_len"] == ref[1]).sum()), int((got["cost"] == ref[0]).sum())
        t_ours, t_theirs = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours, a.reps))
            t_theirs.append(timed(theirs, a.torch_reps))
        print(json.dumps({
            "tool": "dtw_bench", "config": name, "metric": "l1",
            "shape": {"B": B, "Tx": Tx, "Ty": Ty, "C": C, "mean_n": float(xl.float().mean()), "mean_m": float(yl.float().mean())},
            "cells": int((xl * yl).sum()), "rounds": a.rounds, "reps": a.reps, "torch_reps": a.torch_reps,
            "kernels_us": {"min": round(min(t_ours), 1), "median": round(statistics.median(t_ours), 1)},
            "stock_torch_us": {"min": round(min(t_theirs), 1), "median": round(statistics.median(t_theirs), 1)},
            "stock_over_kernels": round(statistics.median(t_theirs) / statistics.median(t_ours), 2),
            "cost_max_rel_diff": rel, "equal_cost": same_cost, "equal_path_len": same_len, "rows": B}), flush=True)


if __name__ == "__main__":
    main()
