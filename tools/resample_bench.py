#!/usr/bin/env python3
"""What the band-limited resampler costs: `Resampler` (csrc/resample.hip) against the same algorithm restated in
stock torch on the same device, alternating round by round in one process.

    python tools/resample_bench.py [--rounds 7] [--reps 20] [--out profiles/resample_bench.txt] [--label TEXT]

Shapes: B = 64 and B = 1 utterances of 6.5 s, all at full length (the stock side knows no lengths), for 48000 -> 22050,
44100 -> 22050 (L = 1) and 16000 -> 22050 (L = 441), and one ragged batch of 64 utterances of 1 s to 6.5 s at 48000 -> 22050
(the stock side resamples the padding).  The stock-torch restatement (tests/resample_reference.py `stock_resample`): pad the
input, `conv1d` with one output channel per phase -- an `(L, 1, K + M - 1)` kernel, phase r's K taps at offset floor(r M / L) of
the window the L outputs of a group share -- at stride M, then transpose, reshape and trim; the weights are the kernel's own
table.  Times: device events around `reps` calls after a warm-up (fewer when a call of the stock side takes more than 50 ms),
the median and minimum over the rounds.  The HBM bound counts 4 B per valid input sample and 4 B per output sample at 8.0 TB/s
(the spec rate) and at 6.3 TB/s (what a copy reaches).  Errors: both sides against the fp64 oracle on the first and the last
utterance.  Prints one JSON line per shape and appends it to `--out` when given."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SECONDS = 6.5
SHAPES = [(48000, 22050, 64, False), (48000, 22050, 1, False), (44100, 22050, 64, False), (44100, 22050, 1, False),
          (16000, 22050, 64, False), (16000, 22050, 1, False), (48000, 22050, 64, True)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def measure(orig, new, B, ragged, args):
    from resample_reference import make_wave, resample_ref, stock_resample, stock_weights
    from transformertts_amd.audio import Resampler
    dev = "cuda:0"
    n = int(round(SECONDS * orig))
    lens = [int(round(orig * (1.0 + (SECONDS - 1.0) * b / max(1, B - 1)))) for b in range(B)] if ragged else [n] * B
    sigs = [make_wave(m, orig, 500 + b) for b, m in enumerate(lens)]
    host = np.zeros((B, n), dtype=np.float32)
    for b, x in enumerate(sigs):
        host[b, :x.size] = x
    wave, wave_lens = torch.from_numpy(host).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
    rs = Resampler(orig, new, device=dev)
    weights = stock_weights(rs.table, rs.L, rs.M, rs.K)
    ours = lambda: rs(wave, wave_lens)["wave"]
    stock = lambda: stock_resample(wave, weights, rs.L, rs.M, rs.K)
    got, ref = ours(), stock()
    assert tuple(got.shape) == tuple(ref.shape) == (B, rs.out_len(n))
    errs = {"kernel": [0.0, 0.0], "stock_torch": [0.0, 0.0]}
    for b in sorted({0, B - 1}):
        want = resample_ref(sigs[b], orig, new)
        for key, y in (("kernel", got), ("stock_torch", ref)):
            d = y[b, :want.size].double().cpu().numpy() - want
            errs[key][0] = max(errs[key][0], float(np.abs(d).max()))
            errs[key][1] = max(errs[key][1], float(np.linalg.norm(d) / np.linalg.norm(want)))
    torch.cuda.synchronize()
    stock_reps = max(1, min(args.reps, int(5e4 / max(1.0, timed(stock, 1)))))
    for _ in range(3):                                               # warm-up: code objects, the convolution's plan, the allocator
        timed(ours, args.reps)
        timed(stock, stock_reps)
    t_ours, t_stock = [], []
    for r in range(args.rounds):                                     # alternating order
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            if which == 0:
                t_ours.append(timed(ours, args.reps))
            else:
                t_stock.append(timed(stock, stock_reps))
    nbytes = 4 * (sum(lens) + B * rs.out_len(n))
    med, med_stock = statistics.median(t_ours), statistics.median(t_stock)
    return {"tool": "resample_bench", "label": args.label,
            "shape": {"orig": orig, "new": new, "B": B, "seconds": "1.0 .. 6.5" if ragged else SECONDS, "samples": n,
                      "outputs": rs.out_len(n), "L": rs.L, "M": rs.M, "K": rs.K},
            "rounds": args.rounds, "reps": {"kernel": args.reps, "stock_torch": stock_reps},
            "kernel_us": {"min": round(min(t_ours), 1), "median": round(med, 1)},
            "stock_torch_us": {"min": round(min(t_stock), 1), "median": round(med_stock, 1)},
            "stock_over_kernel": round(med_stock / med, 2),
            "hbm_bytes": nbytes, "hbm_bound_us": {"at_8.0_TBps": round(nbytes / 8.0e6, 2), "at_6.3_TBps": round(nbytes / 6.3e6, 2)},
            "fraction_of_hbm_bound": {"at_8.0_TBps": round(nbytes / 8.0e6 / med, 4), "at_6.3_TBps": round(nbytes / 6.3e6 / med, 4)},
            "max_abs_err": {k: float(f"{v[0]:.3e}") for k, v in errs.items()},
            "rel_l2_err": {k: float(f"{v[1]:.3e}") for k, v in errs.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="", help="free text carried into every line (which build was measured)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the HIP device: a time is only measured there")
    for orig, new, B, ragged in SHAPES:
        line = json.dumps(measure(orig, new, B, ragged, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
