#!/usr/bin/env python3
"""What the body of the FastSpeech-2 student costs on the library's kernels: the conv feed-forward sublayer of
csrc/predictor.hip forward and forward + backward, an `FFTBlock` forward and forward + backward, and the `FastSpeech2Student`
forward, each against its stock-torch restatement (`where` + `nn.Conv1d` + `layer_norm`, `nn.MultiheadAttention`, the shipped
stock `VariancePredictor`, `repeat_interleave`), both sides alternating round by round in one process.

    python tools/fft_block_bench.py [--rounds 5] [--reps 10] [--out profiles/fft_block_bench.txt] [--label TEXT]

Shapes (d_model 256, hidden 1024, taps 9 and 1, 2 heads): the encoder side at B = 64 utterances of 110 phonemes, the same for
B = 1, a ragged batch of 64 utterances of 20 .. 110 phonemes, and the decoder side at 64 x 870 frames (sublayer and block only;
the student's own decoder runs at the frames its durations give: 8 per phoneme, 880 at most).  Times: device events around
`reps` calls after a warm-up, the median and minimum over the rounds, in microseconds, every call issued from Python (forwards
under `no_grad` in eval mode, forward + backward through autograd in training mode with dropout 0.2).  No ratio is promised:
every cell is printed, `slower_than_stock` lists the cells whose median is above stock's.  Prints one JSON line per shape and
appends it to `--out`."""
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

D, HIDDEN, TAPS, HEADS, DROP = 256, 1024, (9, 1), 2, 0.2
SHAPES = [("encoder_64x110", 64, 110, False, True), ("encoder_1x110", 1, 110, False, True), ("encoder_64x20..110", 64, 110, True, True),
          ("decoder_64x870", 64, 870, False, False)]                 # name, B, rows, ragged, with the student


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


class StockFFN(nn.Module):
    def __init__(self):
        super().__init__()
        self.w_1, self.w_2 = nn.Conv1d(D, HIDDEN, TAPS[0], padding=TAPS[0] // 2), nn.Conv1d(HIDDEN, D, TAPS[1], padding=TAPS[1] // 2)
        self.layer_norm, self.drop = nn.LayerNorm(D), nn.Dropout(DROP)

    def forward(self, x, valid):
        zero = x.new_zeros(())
        xm = torch.where(valid, x, zero)
        h = torch.where(valid, torch.relu(self.w_1(xm.transpose(1, 2)).transpose(1, 2)), zero)
        return torch.where(valid, self.layer_norm(xm + self.drop(self.w_2(h.transpose(1, 2)).transpose(1, 2))), zero)


class StockBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(D, HEADS, dropout=DROP, batch_first=True)
        self.norm, self.drop, self.ffn = nn.LayerNorm(D), nn.Dropout(DROP), StockFFN()

    def forward(self, x, valid):
        a = self.self_attn(x, x, x, key_padding_mask=~valid[:, :, 0], need_weights=False)[0]
        return self.ffn(self.norm(x + self.drop(a)), valid)


class StockStack(nn.Module):
    def __init__(self, n, pe):
        super().__init__()
        self.layers, self.pe = nn.ModuleList(StockBlock() for _ in range(n)), pe

    def forward(self, x, lens):
        valid = (torch.arange(x.size(1), device=x.device)[None, :] < lens[:, None])[:, :, None]
        x = torch.where(valid, x + self.pe[:x.size(1)], x.new_zeros(()))
        for layer in self.layers:
            x = layer(x, valid)
        return x


class StockStudent(nn.Module):
    """the student's training forward in stock torch: same layers, the shipped stock predictors, bucketize, repeat_interleave"""

    def __init__(self, ours):
        super().__init__()
        from transformertts_amd import VariancePredictor
        self.embedding = nn.Embedding(*ours.embedding.weight.shape)
        self.encoder, self.decoder = StockStack(len(ours.encoder.layers), ours.encoder.pe), StockStack(len(ours.decoder.layers), ours.decoder.pe)
        self.predictors = nn.ModuleList(VariancePredictor(D) for _ in range(3))
        e = ours.adaptor.embedding
        self.bins, self.tables = (e.pitch_bins, e.energy_bins), nn.ParameterList([nn.Parameter(e.pitch_table.detach().clone()),
                                                                                  nn.Parameter(e.energy_table.detach().clone())])
        self.mel = nn.Linear(D, ours.mel_linear.out_features)

    def forward(self, phoneme, lens, durations, pitch, energy, max_len):
        x = self.encoder(self.embedding(phoneme), lens)
        preds = [p(x, lens) for p in self.predictors]
        valid = torch.arange(x.size(1), device=x.device)[None, :] < lens[:, None]
        h = torch.where(valid[:, :, None], (x + self.tables[0][torch.bucketize(pitch, self.bins[0])]) + self.tables[1][torch.bucketize(energy, self.bins[1])], x)
        dur = torch.where(valid, durations, torch.zeros_like(durations))
        frames = x.new_zeros(x.size(0), max_len, D)
        for b in range(x.size(0)):
            rows = torch.repeat_interleave(h[b], dur[b], dim=0)[:max_len]
            frames[b, :rows.size(0)] = rows
        mel_lens = dur.sum(1).clamp(max=max_len)
        y = self.decoder(frames, mel_lens)
        return torch.where((torch.arange(max_len, device=x.device)[None, :] < mel_lens[:, None])[:, :, None], self.mel(y), x.new_zeros(())), preds


FRAMES_PER_PHONEME = 8


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from transformertts_amd import ConvFeedForward, FastSpeech2Student, FFTBlock
    dev = "cuda:0"
    torch.manual_seed(0)
    k_ffn, s_ffn = ConvFeedForward(D, HIDDEN, TAPS, DROP).to(dev), StockFFN().to(dev)
    k_blk, s_blk = FFTBlock(D, HEADS, HIDDEN, TAPS, DROP).to(dev), StockBlock().to(dev)
    k_stu = FastSpeech2Student(64, D, 4, 4, HEADS, HIDDEN, TAPS, 80, DROP).to(dev)
    s_stu = StockStudent(k_stu).to(dev)

    def nograd(mod, fn):
        def run():
            mod.eval()
            with torch.no_grad():
                fn()
        return run

    def train(mod, fn):
        def run():
            mod.train()
            fn()
        return run

    for name, B, P, ragged, with_student in SHAPES:
        gen = torch.Generator().manual_seed(7 + B + P + ragged)
        lens_host = [int(round(20 + (P - 20) * b / max(1, B - 1))) for b in range(B)] if ragged else [P] * B
        lens = torch.tensor(lens_host, device=dev)
        valid = (torch.arange(P, device=dev)[None, :] < lens[:, None])[:, :, None]
        x, dy = torch.randn(B, P, D, generator=gen).to(dev), torch.randn(B, P, D, generator=gen).to(dev)
        xg = x.clone().requires_grad_(True)
        cells = {
            "ffn_fwd": (nograd(k_ffn, lambda: k_ffn(x, lens)), nograd(s_ffn, lambda: s_ffn(x, valid))),
            "ffn_fwd+bwd": (train(k_ffn, lambda: k_ffn(xg, lens).backward(dy)), train(s_ffn, lambda: s_ffn(xg, valid).backward(dy))),
            "block_fwd": (nograd(k_blk, lambda: k_blk(x, lens)), nograd(s_blk, lambda: s_blk(x, valid))),
            "block_fwd+bwd": (train(k_blk, lambda: k_blk(xg, lens).backward(dy)), train(s_blk, lambda: s_blk(xg, valid).backward(dy))),
        }
        if with_student:
            ids = torch.randint(1, 64, (B, P), generator=gen).to(dev)
            dur = torch.full((B, P), FRAMES_PER_PHONEME, dtype=torch.int64, device=dev)
            pitch, energy = (200 + 50 * torch.randn(B, P, generator=gen)).to(dev), torch.rand(B, P, generator=gen).to(dev)
            T = FRAMES_PER_PHONEME * P
            cells["student_fwd"] = (nograd(k_stu, lambda: k_stu(ids, lens, durations=dur, pitch=pitch, energy=energy, max_len=T)),
                                    nograd(s_stu, lambda: s_stu(ids, lens, dur, pitch, energy, T)))
        times = {}
        for _ in range(args.rounds):                                  # the two sides alternate inside every round
            for cell, pair in cells.items():
                for side, fn in zip(("kernel", "stock"), pair):
                    fn()
                    times.setdefault((cell, side), []).append(timed(fn, args.reps))
        row = {"tool": "fft_block_bench", "label": args.label, "shape": name, "B": B, "rows": P, "valid_rows": sum(lens_host), "d_model": D,
               "hidden": HIDDEN, "taps": list(TAPS), "heads": HEADS, "rounds": args.rounds, "reps": args.reps,
               "device": torch.cuda.get_device_name(0)}
        for (cell, side), v in times.items():
            row[f"{cell}.{side}.us"] = [round(statistics.median(v), 2), round(min(v), 2)]
        row["slower_than_stock"] = [c for c in cells if statistics.median(times[(c, "kernel")]) > statistics.median(times[(c, "stock")])]
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
