#!/usr/bin/env python3
"""What the variance adaptor costs: the length regulator, the pitch / energy embedding and the three losses of
csrc/variance.hip, forward and backward, against two stock-torch forms on the same device, alternating round by round in one
process.

    python tools/variance_bench.py [--rounds 5] [--reps 20] [--out profiles/variance_bench.txt] [--label TEXT]
    TTTS_LIB=variant.so python tools/variance_bench.py --kernel-only --label "TTTS_LR_FRAMES=16" ...     # another build

Shapes: the flagship's B = 64 utterances of 110 phonemes regulated to 870 frames of D = 256, the same for B = 1, and a ragged
batch of 64 utterances of 20 .. 110 phonemes (frames in proportion).  Stock forms: `loop`, the usual per-utterance
`repeat_interleave` + `pad_sequence` (it reads every utterance's durations back to the host); `vectorised`, `cumsum` +
`searchsorted` + `gather` (its backward is a scatter-add of atomics), with `bucketize` + `nn.functional.embedding` for the
embedding and three masked `mse` for the loss.  Times: device events around `reps` calls after a warm-up, the median and
minimum over the rounds, in microseconds, twice: `us` with every call issued from Python (at these sizes that is mostly the
host: the B = 1 column shows the floor), and `graph_us` with the `reps` calls captured into one HIP graph and replayed, which
is the device's time alone: the forwards under `no_grad`, the kernel side's backwards as the C entries autograd would call
(the loop cannot be captured: it reads durations back; the stock backwards are not, they need the autograd engine).  The regulator's forward is bounded by the
bytes of its output: `out_MB`, the achieved `GBps` (from `graph_us`), and next to it a device-to-device `copy_` of a tensor of
the same size measured the same way in the same rounds.
Prints one JSON line per shape and appends it to `--out` when given."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

P, T, D, BINS = 110, 870, 256, 256
SHAPES = [(64, False), (1, False), (64, True)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def captured(fn, reps):
    """`reps` calls of fn as one HIP graph -> a callable that replays it.  fn must not go through the autograd engine: a backward
    of leaves made on another stream synchronises streams, which a capture does not allow."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    return graph.replay


def make_batch(B, ragged, dev):
    gen = torch.Generator().manual_seed(7 + B + ragged)
    lens = [int(round(20 + (P - 20) * b / max(1, B - 1))) for b in range(B)] if ragged else [P] * B
    dur = torch.zeros(B, P, dtype=torch.int64)
    for b, n in enumerate(lens):
        frames = int(round(T * n / P))
        d = torch.randint(1, 15, (n,), generator=gen).double()
        d = torch.floor(d * (frames / float(d.sum()))).long()
        d[-1] += frames - int(d.sum())                               # the utterance sums to its frames exactly
        dur[b, :n] = d
    x = torch.randn(B, P, D, generator=gen)
    pitch = torch.exp(torch.empty(B, P).uniform_(4.0, 6.5, generator=gen))
    energy = torch.rand(B, P, generator=gen)
    preds = [torch.randn(B, P, generator=gen) for _ in range(3)]
    return [t.to(dev) for t in (x, dur, torch.tensor(lens), pitch, energy, *preds)], lens


def stock_loop(x, dur, lens):
    rows = [torch.repeat_interleave(x[b, :n], dur[b, :n], dim=0) for b, n in enumerate(lens)]
    y = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)
    return torch.nn.functional.pad(y, (0, 0, 0, T - y.size(1)))


def stock_vectorised(x, dur, pl):
    valid = torch.arange(P, device=x.device)[None, :] < pl[:, None]
    c = torch.cumsum(torch.where(valid, dur, torch.zeros_like(dur)), dim=1)
    t = torch.arange(T, device=x.device)[None, :].expand(x.size(0), T).contiguous()
    idx = torch.searchsorted(c, t, right=True).clamp(max=P - 1)
    y = torch.gather(x, 1, idx[:, :, None].expand(-1, -1, x.size(2)))
    return y * (t < c[:, -1:]).to(x.dtype)[:, :, None]


def stock_embed(x, pl, pitch, energy, m):
    valid = (torch.arange(P, device=x.device)[None, :] < pl[:, None])[:, :, None]
    e = torch.nn.functional.embedding(torch.bucketize(pitch, m.pitch_bins), m.pitch_table)
    e2 = torch.nn.functional.embedding(torch.bucketize(energy, m.energy_bins), m.energy_table)
    return torch.where(valid, (x + e) + e2, x)


def stock_loss(preds, dur, pitch, energy, pl):
    valid = torch.arange(P, device=dur.device)[None, :] < pl[:, None]
    n = valid.sum().clamp(min=1)
    terms = [(((p - t) ** 2) * valid).sum() / n for p, t in zip(preds, (torch.log(dur.clamp(min=0).float() + 1.0), pitch, energy))]
    return terms[0] + terms[1] + terms[2]


def measure(B, ragged, args):
    from transformertts_amd import _lib
    from transformertts_amd.variance import VarianceEmbedding, VarianceLoss, length_regulate, variance_bins
    dev = "cuda:0"
    (x, dur, pl, pitch, energy, *preds), lens = make_batch(B, ragged, dev)
    emb = VarianceEmbedding(BINS, BINS, D, pitch_bins=variance_bins(65.0, 600.0, BINS, "log"), energy_bins=variance_bins(0.0, 1.0, BINS)).to(dev)
    loss = VarianceLoss()
    x.requires_grad_(True)
    preds = [p.requires_grad_(True) for p in preds]
    pred = dict(zip(("log_duration", "pitch", "energy"), preds))
    g = torch.randn(B, T, D, device=dev)
    gp = torch.randn(B, P, D, device=dev)
    src, dst = torch.randn(B, T, D, device=dev), torch.empty(B, T, D, device=dev)
    tables = [emb.pitch_table, emb.energy_table]

    def pair(fwd, wrt, grad):
        y = fwd()
        y = y["frames"] if isinstance(y, dict) else y
        return fwd, lambda: torch.autograd.grad(y, wrt, grad, retain_graph=True)

    sides = {
        "kernel": dict(zip(("regulate_fwd", "regulate_bwd"), pair(lambda: length_regulate(x, dur, pl, T), [x], g))),
        "stock_vectorised": dict(zip(("regulate_fwd", "regulate_bwd"), pair(lambda: stock_vectorised(x, dur, pl), [x], g))),
        "stock_loop": dict(zip(("regulate_fwd", "regulate_bwd"), pair(lambda: stock_loop(x, dur, lens), [x], g))),
    }
    sides["kernel"].update(zip(("embed_fwd", "embed_bwd"), pair(lambda: emb(x, pl, pitch=pitch, energy=energy), tables, gp)))
    sides["stock_vectorised"].update(zip(("embed_fwd", "embed_bwd"), pair(lambda: stock_embed(x, pl, pitch, energy, emb), tables, gp)))
    sides["kernel"].update(zip(("loss_fwd", "loss_bwd"), pair(lambda: loss(pred, dur, pitch, energy, pl)["total"], preds, None)))
    sides["stock_vectorised"].update(zip(("loss_fwd", "loss_bwd"), pair(lambda: stock_loss(preds, dur, pitch, energy, pl), preds, None)))
    sides["copy"] = {"regulate_fwd": lambda: dst.copy_(src)}
    if args.kernel_only:
        sides = {k: v for k, v in sides.items() if k in ("kernel", "copy")}
    ours = length_regulate(x, dur, pl, T)
    same = {k: bool(torch.equal(ours["frames"], f(x, dur, pl if k == "stock_vectorised" else lens)))
            for k, f in (("stock_vectorised", stock_vectorised), ("stock_loop", stock_loop)) if k in sides}
    torch.cuda.synchronize()
    times = {side: {op: [] for op in ops} for side, ops in sides.items()}
    from transformertts_amd.ops import _p, _stream
    lib = _lib.load()
    ids = emb(x, pl, pitch=pitch, energy=energy, return_ids=True)
    dx, dtab, gout = torch.empty(B, P, D, device=dev), torch.empty(BINS, D, device=dev), torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)
    dpred = [torch.empty(B, P, device=dev) for _ in range(3)]

    def embed_bwd():
        for k in ("pitch_ids", "energy_ids"):
            _lib.check(lib.ttts_embedding_bwd(_p(ids[k]), _p(gp), _p(dtab), B * P, BINS, D, 0, _stream()), "ttts_embedding_bwd")

    direct = {"regulate_bwd": lambda: _lib.check(lib.ttts_length_regulate_bwd(_p(g), _p(dur), _p(pl), B, P, T, D, _p(dx), 0, _stream()), "bwd"),
              "embed_bwd": embed_bwd,
              "loss_bwd": lambda: _lib.check(lib.ttts_variance_loss_bwd(_p(preds[0]), _p(dur), _p(preds[1]), _p(pitch), _p(preds[2]), _p(energy),
                                                                        _p(pl), B, P, 1.0, 1.0, 1.0, _p(gout), _p(dpred[0]), _p(dpred[1]),
                                                                        _p(dpred[2]), _stream()), "loss_bwd")}
    replays = {side: {op: captured(direct.get(op, fn), args.reps) for op, fn in ops.items() if op.endswith("_fwd") or side == "kernel"}
               for side, ops in sides.items() if side != "stock_loop"}
    gtimes = {side: {op: [] for op in ops} for side, ops in replays.items()}
    for side, ops in sides.items():                                  # warm-up: code objects, the allocator
        for fn in ops.values():
            timed(fn, 3)
    order = list(sides)
    for r in range(args.rounds):                                     # alternating order
        for side in (order if r % 2 == 0 else order[::-1]):
            for op, fn in sides[side].items():
                times[side][op].append(timed(fn, args.reps if side != "stock_loop" else max(1, args.reps // 4)))
                if op in replays.get(side, {}):
                    gtimes[side][op].append(timed(replays[side][op], 3) / args.reps)
    stat = lambda v: {"min": round(min(v), 1), "median": round(statistics.median(v), 1)}
    out_mb = 4 * B * T * D / 1e6
    device = gtimes if "regulate_fwd" in gtimes.get("kernel", {}) and "regulate_fwd" in gtimes.get("copy", {}) else times
    med = statistics.median(device["kernel"]["regulate_fwd"])
    med_copy = statistics.median(device["copy"]["regulate_fwd"])
    line = {"tool": "variance_bench", "label": args.label, "frames_per_workgroup": _lib.load().ttts_length_regulate_frames(),
            "shape": {"B": B, "P": P if not ragged else "20 .. 110", "T": T, "D": D, "bins": BINS, "frames": int(ours["mel_lens"].sum())},
            "rounds": args.rounds, "reps": args.reps,
            "us": {side: {op: stat(v) for op, v in ops.items()} for side, ops in times.items()},
            "graph_us": {side: {op: stat(v) for op, v in ops.items()} for side, ops in gtimes.items()},
            "regulate_fwd": {"out_MB": round(out_mb, 1), "GBps": round(out_mb * 1e3 / med, 1), "copy_GBps": round(out_mb * 1e3 / med_copy, 1),
                             "kernel_over_copy": round(med / med_copy, 2)},
            "same_bits_as": same}
    slower = [f"{key}.{op}" for key, t in (("us", times), ("graph_us", gtimes)) for op, v in t["kernel"].items()
              if op in t.get("stock_vectorised", {}) and statistics.median(v) > statistics.median(t["stock_vectorised"][op])]
    line["slower_than_stock_vectorised"] = slower
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="skip the stock sides (another build of the kernel, see TTTS_LIB)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="", help="free text carried into every line (which build was measured)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("variance_bench needs the HIP device: a time is only measured there")
    for B, ragged in SHAPES:
        line = json.dumps(measure(B, ragged, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
