#!/usr/bin/env python3
"""What a HiFi-GAN generator costs on the library's kernels (csrc/hifigan.hip) against its stock-torch restatement
(`nn.Conv1d` / `nn.ConvTranspose1d` on the padded batch, from the same weights, on the same device), both sides alternating round
by round in one process.

    python tools/hifigan_bench.py [--rounds 5] [--reps 3] [--out profiles/hifigan_bench.txt] [--label TEXT] [--configs v1,v3]

V1 and V3 at 1 x 870 frames and at 16 utterances of 435 .. 870 frames (ragged; stock runs the padded batch, the same work per
utterance as it would do alone at 870).  Times: device events around `reps` calls after a warm-up, the median and minimum over the
rounds, in milliseconds per call, every call issued from Python under `no_grad`.  rtf: seconds of audio (the valid samples at
22050 Hz) per second of device time, from the median.  tflops: 2 Cin Cout taps per output row of every layer (the transposed layers:
taps / stride) over the rows a side computes (the kernels: the valid rows; stock: the padded batch), per second, and its share of
the 157 TF fp32-MFMA peak.  peak_mib: `max_memory_allocated` above what was held before the call.  No ratio is promised:
`slower_than_stock` says which side won.  One JSON line per configuration, appended to `--out`."""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TF, RATE = 157.0, 22050


class StockGenerator(nn.Module):
    """the generator in stock torch, channel-first, state-dict keys as the public checkpoints spell them (plain weights)"""

    def __init__(self, cfg):
        super().__init__()
        c0, self.nk, self.type1 = cfg.upsample_initial_channel, len(cfg.resblock_kernel_sizes), cfg.resblock == "1"
        self.conv_pre = nn.Conv1d(cfg.n_mels, c0, 7, padding=3)
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            self.ups.append(nn.ConvTranspose1d(c0 >> i, c0 >> (i + 1), k, u, padding=(k - u) // 2))
            c = c0 >> (i + 1)
            for kk, dils in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
                blk = nn.Module()
                first = nn.ModuleList(nn.Conv1d(c, c, kk, dilation=d, padding=d * (kk // 2)) for d in dils)
                if self.type1:
                    blk.convs1, blk.convs2 = first, nn.ModuleList(nn.Conv1d(c, c, kk, padding=kk // 2) for _ in dils)
                else:
                    blk.convs = first
                self.resblocks.append(blk)
        self.conv_post = nn.Conv1d(c0 >> len(cfg.upsample_rates), 1, 7, padding=3)

    def block(self, blk, x):
        if self.type1:
            for c1, c2 in zip(blk.convs1, blk.convs2):
                x = x + c2(F.leaky_relu(c1(F.leaky_relu(x, 0.1)), 0.1))
        else:
            for c in blk.convs:
                x = x + c(F.leaky_relu(x, 0.1))
        return x

    def forward(self, mel):
        x = self.conv_pre(mel.transpose(1, 2))
        for i, up in enumerate(self.ups):
            x = up(F.leaky_relu(x, 0.1))
            xs = self.block(self.resblocks[i * self.nk], x)
            for j in range(1, self.nk):
                xs = xs + self.block(self.resblocks[i * self.nk + j], x)
            x = xs / self.nk
        return torch.tanh(self.conv_post(F.leaky_relu(x))).squeeze(1)


def flops_per_frame(cfg):
    """useful floating-point operations per mel frame"""
    ch = cfg.channels
    total, rows = 2.0 * cfg.n_mels * ch[0] * 7, 1
    per_block = 2 if cfg.resblock == "1" else 1
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        total += rows * 2.0 * ch[i] * ch[i + 1] * k                      # per input row: every tap of the transposed layer once
        rows *= u
        for kk, dils in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
            total += rows * len(dils) * per_block * 2.0 * ch[i + 1] * ch[i + 1] * kk
    return total + rows * 2.0 * ch[-1] * 7


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--configs", default="v1,v3")
    ap.add_argument("--frames", type=int, default=870)
    args = ap.parse_args()
    from transformertts_amd import HiFiGANConfig, HiFiGANGenerator
    dev = "cuda:0"
    for preset in args.configs.split(","):
        cfg = {"v1": HiFiGANConfig.v1, "v3": HiFiGANConfig.v3}[preset]()
        torch.manual_seed(0)
        stock = StockGenerator(cfg)
        with torch.no_grad():
            for name, p in stock.named_parameters():                     # fan-in scale: activations of order one through the depth
                if p.dim() == 3:
                    fan = p.shape[1] * p.shape[2] if not name.startswith("ups.") else p.shape[0] * p.shape[2] / cfg.upsample_rates[int(name.split(".")[1])]
                    p.copy_(torch.randn_like(p) / fan ** 0.5)
        sd = {k: v.detach().clone() for k, v in stock.state_dict().items()}
        stock = stock.to(dev).eval()
        kernels = HiFiGANGenerator(cfg, sd, device=dev)
        for B in (1, 16):
            T = args.frames
            lens_host = [T - (T // 2) * b // max(1, B - 1) for b in range(B)] if B > 1 else [T]
            lens = torch.tensor(lens_host, device=dev)
            mel = torch.randn(B, T, cfg.n_mels, generator=torch.Generator().manual_seed(B)).to(dev)

            def run_kernels():
                with torch.no_grad():
                    return kernels(mel, lens)["wave"]

            def run_stock():
                with torch.no_grad():
                    return stock(mel)

            # the two sides agree on the utterance that fills the batch (no padding leaks into it)
            full = lens_host.index(T)
            a, b = run_kernels()[full], run_stock()[full]
            agree = float((a - b).norm() / b.norm())
            times = {"kernel": [], "stock": []}
            for _ in range(args.rounds):                                 # the two sides alternate inside every round
                for side, fn in (("kernel", run_kernels), ("stock", run_stock)):
                    fn()
                    times[side].append(timed(fn, args.reps))
            mem = {"kernel": peak_mib(run_kernels), "stock": peak_mib(run_stock)}
            frames = sum(lens_host)
            row = {"tool": "hifigan_bench", "label": args.label, "config": preset, "B": B, "frames": T, "valid_frames": frames,
                   "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0), "rel_l2_full_utterance": agree,
                   "gflop_valid": round(flops_per_frame(cfg) * frames / 1e9, 1), "predicted_peak_mib": round(kernels.peak_bytes(B, T) / 2 ** 20, 1)}
            for side, v in times.items():
                med = statistics.median(v)
                work = flops_per_frame(cfg) * (frames if side == "kernel" else B * T)      # stock computes the padding too
                row[f"{side}.ms"] = [round(med, 3), round(min(v), 3)]
                row[f"{side}.rtf"] = round(frames * cfg.hop / RATE / (med * 1e-3), 1)
                row[f"{side}.tflops"] = round(work / (med * 1e-3) / 1e12, 2)
                row[f"{side}.share_of_peak"] = round(work / (med * 1e-3) / 1e12 / PEAK_TF, 3)
                row[f"{side}.peak_mib"] = mem[side]
            row["slower_than_stock"] = statistics.median(times["kernel"]) > statistics.median(times["stock"])
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
