#!/usr/bin/env python3
"""What the Griffin-Lim vocoder costs: `Vocoder.griffin_lim` (csrc/vocoder.hip) against the same algorithm restated
in stock torch on the same device (`torch.istft` / `torch.stft`, the same `init` and `momentum`), alternating round by round in
one process.

    python tools/vocoder_bench.py [--rounds 5] [--reps 3] [--n-iter 32] [--seconds 6.5] [--out profiles/vocoder_bench.txt]
    python tools/vocoder_bench.py --profile-run        # a few calls at B = 64 and nothing else: the target of
                                                       # rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python ...

Shapes: B = 1 and B = 64 utterances of 6.5 s at the shipped config (22 050 Hz, n_fft 1024, hop 256), all at full length, and a
ragged batch of 64 whose lengths run evenly from 1 s to 6.5 s (the stock side knows no lengths and does the full rectangle; the
kernels skip what lies behind a length).  The target magnitudes are the front end's spectrogram of tests/audio_reference.py's
signal.  Times: device events around `reps` calls after a warm-up, median and minimum over the rounds; the two transform
kernels also on their own (events around 20 launches each), and the whole call replayed from one HIP graph.  Per launch the
tool states what each transform kernel must move through HBM (spectrum, magnitudes, previous spectrum, wave; once each) and
through LDS (the FFT stages, the fold / unpacking and the overlap-add of every frame, halo frames included), and the times those
take at 6.3 TB/s (what a copy reaches) and at 128 B per clock and CU of 4-byte LDS accesses (256 CUs at 2.4 GHz).  The spectral
convergence of both results is taken with torch.stft in fp64.  One JSON line per shape, appended to `--out` when given."""
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
LDS_BYTES_PER_US = 128 * 256 * 2400.0        # 4-byte accesses: 128 B per clock and CU, 256 CUs, 2.4 GHz
HBM_BYTES_PER_US = 6.3e6


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def stock_griffin_lim(mag, init, cfg, window, n_iter, momentum):
    n_fft, hop, win = cfg["n_fft"], cfg["hop_length"], cfg["win_length"]
    length = (mag.size(1) - 1) * hop
    magT = mag.transpose(1, 2)
    spec = magT * init.transpose(1, 2)                                # (B, bins, T)
    prev = torch.zeros_like(spec)
    c = momentum / (1.0 + momentum)
    one = torch.ones((), dtype=spec.dtype, device=spec.device)
    for _ in range(n_iter):
        wave = torch.istft(spec, n_fft, hop_length=hop, win_length=win, window=window, center=True, length=length)
        reb = torch.stft(wave, n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect", return_complex=True)
        t = reb - c * prev
        prev = reb
        a = t.abs()
        spec = magT * torch.where(a * a > 1e-30, t / a.clamp_min(1e-30), one)
    return torch.istft(spec, n_fft, hop_length=hop, win_length=win, window=window, center=True, length=length)


def spectral_convergence(wave, lens, mag, frames, cfg):
    """|| |STFT(wave)| - mag || / || mag || over the valid frames, torch.stft in fp64"""
    num = den = 0.0
    w = torch.hann_window(cfg["win_length"], periodic=True, dtype=torch.float64, device=wave.device)
    for b in range(0, wave.size(0), max(1, wave.size(0) // 4)):      # a few rows are enough for a figure
        n, T = int(lens[b]), int(frames[b])
        s = torch.stft(wave[b, :n].double(), cfg["n_fft"], hop_length=cfg["hop_length"], win_length=cfg["win_length"], window=w,
                       center=True, pad_mode="reflect", return_complex=True).abs().T
        num += float(((s - mag[b, :T].double()) ** 2).sum())
        den += float((mag[b, :T].double() ** 2).sum())
    return (num / den) ** 0.5


def fft_lds_bytes(M):
    """bytes one M-point fft_lds moves through LDS: per stage every point read and written (re, im) and the twiddles"""
    total, ns = 0, 1
    while ns < M:
        r = 4 if M // ns >= 4 else 2
        total += 2 * M * 4 * 2
        if ns > 1:
            total += (r - 1) * (M // r) * 2 * 4
        ns *= r
    return total


def traffic(B, frames, cfg, span_mult):
    """(HBM bytes, LDS bytes) of one inverse and of one projection launch over the valid frames"""
    n_fft, hop = cfg["n_fft"], cfg["hop_length"]
    M, bins = n_fft // 2, n_fft // 2 + 1
    T = int(sum(frames))
    samples = int(sum(max(f - 1, 0) * hop for f in frames))
    span = span_mult * n_fft
    halo = -(-n_fft // hop) - 1
    computed = int(sum(f + halo * max(0, -(-(max(f - 1, 0) * hop) // span) - 1) for f in frames))   # halo frames are done twice
    per_frame_inv = 2 * M * 4 + M * 4 + fft_lds_bytes(M) + 2 * M * 4 + 3 * n_fft * 4      # fold writes, w^k, FFT, result reads, add (r+w) + span
    per_frame_fwd = 2 * M * 4 + fft_lds_bytes(M) + 2 * M * 4 * 2 + M * 4                   # frame writes, FFT, unpack reads (k and M-k), w^k
    inv = (T * bins * 8 + samples * 4, computed * per_frame_inv + samples * 4)
    fwd = (samples * 4 + T * bins * (4 + 8 + 8 + 8), T * per_frame_fwd)
    return {"istft": inv, "stft_project": fwd, "frames": T, "frames_computed_by_istft": computed}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.99)
    ap.add_argument("--seconds", type=float, default=6.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="only the two per-launch times at B = 64 (span comparisons)")
    ap.add_argument("--span-mult", type=int, default=None, help="the span of the library under TTTS_LIB when it is not the shipped one")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vocoder_bench needs the HIP device: a time is only measured there")
    from audio_reference import make_signal
    from transformertts_amd import _lib, audio
    from transformertts_amd.ops import _p, _stream
    cfg, dev = CONFIG, "cuda:0"
    hop = cfg["hop_length"]
    n = int(round(args.seconds * cfg["sample_rate"]))
    voc = audio.Vocoder(cfg, device=dev, n_iter=args.n_iter, momentum=args.momentum)
    window = torch.hann_window(cfg["win_length"], periodic=True, dtype=torch.float32, device=dev)
    sigs = np.stack([make_signal(n, cfg["sample_rate"], 900 + b) for b in range(64)])
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def shape(B, ragged):
        wave = torch.from_numpy(sigs[:B]).to(dev)
        lens = torch.linspace(cfg["sample_rate"], n, B).long().to(dev) if ragged else torch.full((B,), n, dtype=torch.int64, device=dev)
        m = voc.front_end.spectrogram(wave, lens)
        mag, frames = m["spectrogram"], m["melspec_lens"]
        init = torch.polar(torch.ones_like(mag), torch.rand(mag.shape, generator=gen, device=dev) * (2 * np.pi))
        return mag, frames, init

    if args.profile_run:
        mag, frames, init = shape(64, False)
        for _ in range(3):
            voc.griffin_lim(mag, frames, init=init)
        torch.cuda.synchronize()
        return

    for B, ragged in ((64, False),) if args.kernels_only else ((1, False), (64, False), (64, True)):
        mag, frames, init = shape(B, ragged)
        T = mag.size(1)
        ours = lambda: voc.griffin_lim(mag, frames, init=init)
        stock = lambda: stock_griffin_lim(mag, init, cfg, window, args.n_iter, args.momentum)
        # the two transform kernels on their own
        spec = torch.view_as_real(init * mag).contiguous()
        prev = torch.zeros_like(spec)
        wave, wave_lens = voc._istft(spec, frames, B, T)
        Nmax, lib, tables = (T - 1) * hop, _lib.load(), voc.front_end.tables
        inv = lambda: lib.ttts_istft(_p(spec), _p(frames), B, T, cfg["n_fft"], hop, _p(tables), _p(wave), _p(wave_lens), _stream())
        fwd = lambda: lib.ttts_stft_project(_p(wave), Nmax, None, _p(frames), B, Nmax, cfg["n_fft"], hop, _p(tables), _p(mag), _p(prev),
                                            args.momentum, _p(spec), None, _stream())
        for _ in range(2):
            timed(inv, 20), timed(fwd, 20)
        t_inv = [timed(inv, 20) for _ in range(args.rounds)]
        t_fwd = [timed(fwd, 20) for _ in range(args.rounds)]
        tr = traffic(B, frames.tolist(), cfg, args.span_mult or audio.SPAN_MULT)
        per_kernel = {}
        for key, ts in (("istft", t_inv), ("stft_project", t_fwd)):
            med = statistics.median(ts)
            hbm, lds = tr[key]
            per_kernel[key] = {"us": {"min": round(min(ts), 1), "median": round(med, 1)}, "hbm_bytes": hbm, "lds_bytes": lds,
                               "hbm_us_at_6.3_TBps": round(hbm / HBM_BYTES_PER_US, 1), "lds_us_at_128_B_per_clk_cu": round(lds / LDS_BYTES_PER_US, 1),
                               "hbm_share": round(hbm / HBM_BYTES_PER_US / med, 3), "lds_share": round(lds / LDS_BYTES_PER_US / med, 3)}
        res = {"tool": "vocoder_bench", "library": os.path.basename(_lib.LIB_PATH), "span_mult": args.span_mult or audio.SPAN_MULT,
               "shape": {"B": B, "ragged": ragged, "Tmax": T, "frames": tr["frames"], "frames_computed_by_istft": tr["frames_computed_by_istft"],
                         "n_iter": args.n_iter, "momentum": args.momentum, **{k: cfg[k] for k in ("sample_rate", "n_fft", "hop_length")}},
               "per_launch": per_kernel}
        if not args.kernels_only:
            got, ref = ours(), stock()
            lens = got["wave_lens"]
            res["spectral_convergence"] = {"kernel": round(spectral_convergence(got["wave"], lens, mag, frames, cfg), 6),
                                           "stock_torch": round(spectral_convergence(ref, lens, mag, frames, cfg), 6)}
            for _ in range(2):                                           # warm-up: code objects, rocFFT plans, the allocator
                timed(ours, args.reps), timed(stock, args.reps)
            t_ours, t_stock = [], []
            for r in range(args.rounds):                                 # alternating order
                for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                    (t_ours if which == 0 else t_stock).append(timed(ours if which == 0 else stock, args.reps))
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                ours()
            timed(g.replay, args.reps)
            t_graph = [timed(g.replay, args.reps) for _ in range(args.rounds)]
            med = statistics.median(t_ours)
            transforms = (args.n_iter + 1) * statistics.median(t_inv) + args.n_iter * statistics.median(t_fwd)
            res.update({"rounds": args.rounds, "reps": args.reps,
                        "kernel_us": {"min": round(min(t_ours), 1), "median": round(med, 1)},
                        "kernel_graph_us": {"min": round(min(t_graph), 1), "median": round(statistics.median(t_graph), 1)},
                        "stock_torch_us": {"min": round(min(t_stock), 1), "median": round(statistics.median(t_stock), 1)},
                        "stock_over_kernel": round(statistics.median(t_stock) / med, 2),
                        "transform_launches_us": round(transforms, 1),
                        "split": {"istft": round((args.n_iter + 1) * statistics.median(t_inv) / transforms, 3),
                                  "stft_project": round(args.n_iter * statistics.median(t_fwd) / transforms, 3)}})
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
