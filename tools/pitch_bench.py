#!/usr/bin/env python3
"""What frame pitch and energy cost: `PitchEnergy` (csrc/pitch.hip) against the same algorithm restated in stock
torch on the same device, alternating round by round in one process.

    python tools/pitch_bench.py [--rounds 5] [--reps 20] [--chunk 512] [--out profiles/pitch_bench.txt] [--label TEXT]
    TTTS_LIB=variant.so python tools/pitch_bench.py --kernel-only --label "TTTS_PITCH_LAGS=1" ...      # another build of the kernel

Shapes at the shipped config (22050 Hz, hop 256, n_fft = frame 1024, window 512, lags 36 .. 340): B = 64 and B = 1 utterances
of 6.5 s at full length (the stock side knows no lengths), and the ragged batch of the other audio benches, 64 utterances of
1 s to 6.5 s (the stock side works on the padding).  The stock-torch restatement: reflect-pad, `unfold` into frames, and per
chunk of `--chunk` frames `unfold` again into the (frames, tau_max, W) tensor of shifted windows, subtract, square, sum; cumsum,
the first crossing, the walk and the argmin as masks and argmax; the parabola; the energy from `torch.stft`.  Times: device
events around `reps` calls after a warm-up (fewer when a call of the stock side takes more than 50 ms), the median and minimum
over the rounds.  `pairs` is frames * tau_max * W by the definition (valid frames only), `pairs_per_us` that over the kernel's
median.  Errors: both sides against the fp64 oracle on the first utterance (voicing flips on decided frames, f0 in cents).
Prints one JSON line per shape and appends it to `--out` when given."""
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
CONFIG = dict(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80, fmin=0.0, fmax=8000.0)
SHAPES = [(64, False), (1, False), (64, True)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def stock_pitch(wave, pe, chunk):
    """(B, N) full-length rows -> f0, voiced, aperiodicity, energy (B, T) in stock torch, YIN as csrc/pitch.hip defines it"""
    B, N = wave.shape
    F, W, hop, lo, hi = pe.frame_length, pe.window, pe.hop, pe.tau_min, pe.tau_max
    padded = torch.nn.functional.pad(wave[:, None], (F // 2, F // 2), mode="reflect")[:, 0]
    fr = padded.unfold(1, F, hop).reshape(-1, F)                     # (B T, F)
    taus = torch.arange(1, hi + 1, device=wave.device, dtype=torch.float32)
    idx = torch.arange(1, hi + 1, device=wave.device)
    f0s, vs, aps = [], [], []
    for a in range(0, fr.size(0), chunk):
        x = fr[a:a + chunk]
        d = ((x[:, None, :W] - x.unfold(1, W, 1)[:, 1:hi + 1]) ** 2).sum(-1)             # (C, tau_max)
        cs = torch.cumsum(d, dim=1)
        dp = torch.where(cs == 0, torch.ones_like(d), d * taus / torch.where(cs == 0, torch.ones_like(cs), cs))
        below = (dp < pe.threshold) & (idx >= lo)
        voiced = below.any(dim=1)
        tau0 = torch.argmax(below.to(torch.int8), dim=1) + 1
        stop = torch.cat([~(dp[:, 1:] < dp[:, :-1]), torch.ones_like(dp[:, :1], dtype=torch.bool)], dim=1) & (idx[None, :] >= tau0[:, None])
        walked = torch.argmax(stop.to(torch.int8), dim=1) + 1
        lowest = torch.argmin(dp[:, lo - 1:], dim=1) + lo
        tau = torch.where(voiced, walked, lowest)
        g = lambda t: dp.gather(1, (t - 1).clamp(0, hi - 1)[:, None])[:, 0]
        pa, pb, pc = g(tau - 1), g(tau), g(tau + 1)
        den = pa - 2.0 * pb + pc
        inner = (tau > lo) & (tau < hi) & (den > 0)
        shift = torch.where(inner, (0.5 * (pa - pc) / torch.where(inner, den, torch.ones_like(den))).clamp(-0.5, 0.5), torch.zeros_like(den))
        f0s.append(torch.where(voiced, pe.sample_rate / (tau.to(torch.float32) + shift), torch.zeros_like(den)))
        vs.append(voiced)
        aps.append(pb)
    win = pe.hann
    spec = torch.stft(wave, pe.n_fft, hop_length=hop, win_length=pe.n_fft, window=win, center=True, pad_mode="reflect", return_complex=True)
    energy = (spec.real ** 2 + spec.imag ** 2).sum(dim=1).sqrt()
    T = 1 + N // hop
    return torch.cat(f0s).view(B, T), torch.cat(vs).view(B, T), torch.cat(aps).view(B, T), energy


def measure(B, ragged, args):
    from pitch_reference import SHIPPED, cents, glide_signal, pitch_ref
    from transformertts_amd import _lib
    from transformertts_amd.audio import PitchEnergy
    dev = "cuda:0"
    sr = CONFIG["sample_rate"]
    n = int(round(SECONDS * sr))
    lens = [int(round(sr * (1.0 + (SECONDS - 1.0) * b / max(1, B - 1)))) for b in range(B)] if ragged else [n] * B
    sigs = [glide_signal(m, SHIPPED, 500 + b) for b, m in enumerate(lens)]
    host = np.zeros((B, n), dtype=np.float32)
    for b, x in enumerate(sigs):
        host[b, :x.size] = x
    wave, wave_lens = torch.from_numpy(host).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
    pe = PitchEnergy(CONFIG, device=dev)
    ours = lambda: pe(wave, wave_lens)
    stock = lambda: stock_pitch(wave, pe, args.chunk)
    got = ours()
    ref = pitch_ref(sigs[0], SHIPPED)
    T0 = ref["frames"]
    ok = ref["margin"] > 1e-5
    v = ok & ref["voiced"]
    sides = {"kernel": (got["f0"][0, :T0].cpu().numpy(), got["voiced"][0, :T0].cpu().numpy())}
    if not args.kernel_only:
        s = stock()
        sides["stock_torch"] = (s[0][0, :T0].cpu().numpy(), s[1][0, :T0].cpu().numpy())
    errs = {k: {"voicing_flips_on_decided": int((vo[ok] != ref["voiced"][ok]).sum()),
                "f0_cents_max": float(f"{cents(np.where(vo[v], f0[v], 1.0), ref['f0'][v]).max():.3e}")} for k, (f0, vo) in sides.items()}
    torch.cuda.synchronize()
    for _ in range(3):                                               # warm-up: code objects, the allocator
        timed(ours, args.reps)
    t_ours, t_stock, stock_reps = [], [], 0
    if args.kernel_only:
        t_ours = [timed(ours, args.reps) for _ in range(args.rounds)]
    else:
        stock_reps = max(1, min(args.reps, int(5e4 / max(1.0, timed(stock, 1)))))
        timed(stock, stock_reps)
        for r in range(args.rounds):                                 # alternating order
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                if which == 0:
                    t_ours.append(timed(ours, args.reps))
                else:
                    t_stock.append(timed(stock, stock_reps))
    frames = int(got["frames"].sum())
    pairs = frames * pe.tau_max * pe.window
    med = statistics.median(t_ours)
    lib = _lib.load()
    line = {"tool": "pitch_bench", "label": args.label, "lags_per_thread": lib.ttts_pitch_lags(),
            "frames_per_workgroup": lib.ttts_pitch_frames(pe.n_fft, pe.hop, pe.frame_length, pe.window, pe.tau_max),
            "shape": {"B": B, "seconds": "1.0 .. 6.5" if ragged else SECONDS, "samples": n, "frames": frames, "tau_max": pe.tau_max,
                      "window": pe.window, "hop": pe.hop},
            "rounds": args.rounds, "reps": {"kernel": args.reps, "stock_torch": stock_reps},
            "kernel_us": {"min": round(min(t_ours), 1), "median": round(med, 1)}, "pairs": pairs, "pairs_per_us": round(pairs / med, 1),
            "errors_utterance_0": errs}
    if t_stock:
        med_stock = statistics.median(t_stock)
        line["stock_torch_us"] = {"min": round(min(t_stock), 1), "median": round(med_stock, 1)}
        line["stock_over_kernel"] = round(med_stock / med, 2)
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=512, help="frames per (frames, tau_max, W) tensor of the stock side")
    ap.add_argument("--kernel-only", action="store_true", help="skip the stock side (another build of the kernel, see TTTS_LIB)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="", help="free text carried into every line (which build was measured)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench needs the HIP device: a time is only measured there")
    for B, ragged in SHAPES:
        line = json.dumps(measure(B, ragged, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
