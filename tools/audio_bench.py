#!/usr/bin/env python3
"""What the log-mel front end costs: `MelFrontEnd` (csrc/audio.hip) against the same computation restated in stock
torch on the same device, alternating round by round in one process.

    python tools/audio_bench.py [--rounds 7] [--reps 20] [--batch 64] [--seconds 6.5] [--out profiles/audio_bench.txt]

B = 64 utterances of 6.5 s at the shipped config (22 050 Hz, n_fft 1024, hop 256, 80 mels, 0 .. 8000 Hz), all at full length, so
the stock side (which knows no lengths) does the same work.  The stock-torch restatement: `torch.stft(center=True,
pad_mode='reflect', window=hann_window(periodic=True))`, `.abs()`, a dense `(80 x 513)` matmul, `log(clamp(min=1e-5))` and the
transpose to the `(B, T, n_mels)` layout the model takes.  Times: device events around `reps` calls after a warm-up, the median
and minimum over the rounds.  The HBM bound counts 4 B per sample in and `n_mels * 4 / hop` B per sample out at 8.0 TB/s (the
spec rate) and at 6.3 TB/s (what a copy reaches).  Errors: both sides against the fp64 oracle of tests/audio_reference.py on the
first and the last utterance (the input is that file's test signal, zeros from sample 1500 to 2999 of every utterance
included).  Prints one JSON line and appends it to `--out` when given."""
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

CONFIG = dict(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80, fmin=0.0, fmax=8000.0)
CLIP = 1e-5


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def stock_logmel(wave, cfg, window, fb):
    spec = torch.stft(wave, cfg["n_fft"], hop_length=cfg["hop_length"], win_length=cfg["win_length"], window=window, center=True,
                      pad_mode="reflect", return_complex=True).abs()                    # (B, bins, T)
    return torch.log(torch.clamp(torch.matmul(fb, spec), min=CLIP)).transpose(1, 2).contiguous()


def hbm_bytes(B, n, cfg):
    """what the algorithm must move: every sample once in, every mel value once out"""
    return B * n * 4 + B * (1 + n // cfg["hop_length"]) * cfg["n_mels"] * 4


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=6.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("audio_bench needs the HIP device: a time is only measured there")
    from audio_reference import logmel_ref, make_signal
    from transformertts_amd.audio import MelFrontEnd, mel_filterbank
    cfg, dev = CONFIG, "cuda:0"
    B, n = args.batch, int(round(args.seconds * cfg["sample_rate"]))
    sigs = [make_signal(n, cfg["sample_rate"], 900 + b, zero=(1500, 3000)) for b in range(B)]
    wave = torch.from_numpy(np.stack(sigs)).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    fe = MelFrontEnd(cfg, device=dev)
    window = torch.hann_window(cfg["win_length"], periodic=True, dtype=torch.float32, device=dev)
    fb = torch.from_numpy(mel_filterbank(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])).float().to(dev)
    ours = lambda: fe(wave, lens)["melspec"]
    stock = lambda: stock_logmel(wave, cfg, window, fb)

    got, ref = ours(), stock()
    T = 1 + n // cfg["hop_length"]
    assert tuple(got.shape) == tuple(ref.shape) == (B, T, cfg["n_mels"])
    errs = {"kernel": [0.0, 0.0], "stock_torch": [0.0, 0.0]}
    for b in (0, B - 1):
        want = logmel_ref(sigs[b], cfg)
        for key, x in (("kernel", got), ("stock_torch", ref)):
            d = x[b].double().cpu().numpy() - want
            errs[key][0] = max(errs[key][0], float(np.abs(d).max()))
            errs[key][1] = max(errs[key][1], float(np.linalg.norm(d) / np.linalg.norm(want)))
    for _ in range(3):                                               # warm-up: code objects, rocFFT plans, the allocator
        timed(ours, args.reps)
        timed(stock, args.reps)
    t_ours, t_stock = [], []
    for r in range(args.rounds):                                     # alternating order
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            (t_ours if which == 0 else t_stock).append(timed(ours if which == 0 else stock, args.reps))
    nbytes = hbm_bytes(B, n, cfg)
    med = statistics.median(t_ours)
    res = {"tool": "audio_bench", "shape": {"B": B, "samples": n, "frames": T, **cfg}, "rounds": args.rounds, "reps": args.reps,
           "kernel_us": {"min": round(min(t_ours), 1), "median": round(med, 1)},
           "stock_torch_us": {"min": round(min(t_stock), 1), "median": round(statistics.median(t_stock), 1)},
           "stock_over_kernel": round(statistics.median(t_stock) / med, 2),
           "hbm_bytes": nbytes, "hbm_bound_us": {"at_8.0_TBps": round(nbytes / 8.0e6, 2), "at_6.3_TBps": round(nbytes / 6.3e6, 2)},
           "fraction_of_hbm_bound": {"at_8.0_TBps": round(nbytes / 8.0e6 / med, 4), "at_6.3_TBps": round(nbytes / 6.3e6 / med, 4)},
           "logmel_max_abs_err": {k: float(f"{v[0]:.3e}") for k, v in errs.items()},
           "logmel_rel_l2_err": {k: float(f"{v[1]:.3e}") for k, v in errs.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
