#!/usr/bin/env python3
"""A directory of recordings -> the `.npz` files `TransformerTTSDataset` trains from (the mel half of the reference's
`preprocess.py:28-72`), through `MelFrontEnd` (csrc/audio.hip).

    python tools/preprocess_mel.py --config config.yaml [--batch 64] [--sequences DIR] [--stats stats.json] [--resample] [--prosody]

Reads `config['path']['data']/wavs/*.wav` (mono; at `config['audio']['sample_rate']`, or with `--resample` at any rate: the
recordings of a batch that are at another rate are grouped by their rate and brought to the config's on the device by
`audio.Resampler`, csrc/resample.hip, one resampler per distinct rate, before the front end; without the flag such a file is
refused as before) and writes one `<id>.npz` per recording into `config['path']['preprocessed']`.  With `config['audio']['normalize_mel']` a first pass over the
batches adds sum, sum of squares and count of the unnormalised log-mels, mean = S / n, std = sqrt(Q / n - mean^2 + 1e-8), written
to the `--stats` file with the keys `mean` and `std`; the second pass writes `melspec (n_mels, T)` fp32, normalised with them.
Phonemisation is not done here (it needs `g2p_en`): `--sequences DIR` copies `transcript`, `phoneme` and `sequence` from the
`<id>.npz` of DIR (files written by the reference's preprocess.py); without it only `melspec` is written, which the data set
cannot train from yet, and the tool says so.  A recording of n_fft/2 samples or fewer cannot be framed and is skipped.
`--prosody` adds the frame-level targets of a FastSpeech-2-style student to each file, from `audio.PitchEnergy` (csrc/pitch.hip) on
the same uploaded batch and the front end's window table: `f0` (fp32, Hz, 0 where unvoiced), `voiced` (bool) and `energy` (fp32),
each cut to the utterance's frames (the columns of `melspec`)."""
import argparse
import glob
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from transformertts_amd import audio  # noqa: E402


def make_front_end(audio_config):
    return audio.MelFrontEnd(audio_config)


def make_resampler(orig_rate, new_rate):
    return audio.Resampler(orig_rate, new_rate)


def make_pitch_energy(audio_config, front_end):
    return audio.PitchEnergy(audio_config, front_end=front_end)


def _pad(sigs):
    wave = np.zeros((len(sigs), max(s.size for s in sigs)), dtype=np.float32)
    for b, s in enumerate(sigs):
        wave[b, :s.size] = s
    return wave


def read_resampled(paths, sample_rate, resamplers):
    """the recordings at `sample_rate`: those at another rate go, one padded batch per native rate, through that rate's
    resampler (made on first use and kept in `resamplers`)"""
    sigs, by_rate = [None] * len(paths), {}
    for i, p in enumerate(paths):
        x, rate = audio.read_wav_native(p)
        if rate == int(sample_rate) or x.size == 0:
            sigs[i] = x
        else:
            by_rate.setdefault(rate, []).append((i, x))
    for rate, group in sorted(by_rate.items()):
        if rate not in resamplers:
            resamplers[rate] = make_resampler(rate, int(sample_rate))
        rs = resamplers[rate]
        wave = torch.from_numpy(_pad([x for _, x in group]))
        out = rs(wave if rs.device is None else wave.to(rs.device), torch.tensor([x.size for _, x in group], dtype=torch.int64))
        res, lens = out["wave"].cpu().numpy(), out["wave_lens"].cpu().numpy()
        for b, (i, _) in enumerate(group):
            sigs[i] = np.ascontiguousarray(res[b, :int(lens[b])], dtype=np.float32)
    return sigs


def batches(paths, batch, sample_rate, min_len, log, resample=False, resamplers=None):
    """-> (ids, wave (B, Nmax) fp32 zero padded, lens) per batch of recordings long enough to frame"""
    resamplers = {} if resamplers is None else resamplers
    for a in range(0, len(paths), batch):
        ids, sigs = [], []
        chunk = paths[a:a + batch]
        loaded = read_resampled(chunk, sample_rate, resamplers) if resample else None
        for i, p in enumerate(chunk):
            x = loaded[i] if resample else audio.read_wav(p, sample_rate)
            if x.size < min_len:
                log(f"skipped {p}: {x.size} samples, {min_len} needed")
                continue
            ids.append(os.path.splitext(os.path.basename(p))[0])
            sigs.append(x)
        if not ids:
            continue
        yield ids, _pad(sigs), [s.size for s in sigs]


def global_stats(fe, paths, batch, sample_rate, min_len, log, resample=False, resamplers=None):
    total = total_sq = 0.0
    count = 0
    for _, wave, lens in batches(paths, batch, sample_rate, min_len, log, resample, resamplers):
        out = fe(torch.from_numpy(wave).to(fe.device), torch.tensor(lens, dtype=torch.int64))
        s, q, n = fe.stats(out["melspec"], out["melspec_lens"])
        total, total_sq, count = total + float(s), total_sq + float(q), count + int(n)
    if count == 0:
        raise RuntimeError("no recording could be framed")
    mean = total / count
    return mean, math.sqrt(total_sq / count - mean ** 2 + 1e-8)


def run(config, batch=64, sequences=None, stats_path="stats.json", log=print, resample=False, prosody=False):
    a = config["audio"]
    out_dir = config["path"]["preprocessed"]
    paths = sorted(glob.glob(os.path.join(config["path"]["data"], "wavs", "*.wav")))
    if not paths:
        raise RuntimeError(f"no .wav under {os.path.join(config['path']['data'], 'wavs')}")
    os.makedirs(out_dir, exist_ok=True)
    fe = make_front_end(a)
    min_len = int(a["n_fft"]) // 2 + 1
    resamplers = {}                                                   # one per distinct native rate, shared by both passes
    if a.get("normalize_mel"):
        mean, std = global_stats(fe, paths, batch, a["sample_rate"], min_len, lambda m: None, resample, resamplers)
        with open(stats_path, "w", encoding="utf-8") as f:
            json.dump({"mean": mean, "std": std}, f, ensure_ascii=False, indent=2)
        log(f"mean {mean:.6f} std {std:.6f} -> {stats_path}")
        fe.set_stats(mean, std)
    if sequences is None:
        log("no --sequences: the files hold `melspec` only; TransformerTTSDataset also needs `transcript` and `sequence`")
    pe = make_pitch_energy(a, fe) if prosody else None
    written = 0
    for ids, wave, lens in batches(paths, batch, a["sample_rate"], min_len, log, resample, resamplers):
        wave_dev, lens_host = torch.from_numpy(wave).to(fe.device), torch.tensor(lens, dtype=torch.int64)
        out = fe(wave_dev, lens_host)
        mel, mel_lens = out["melspec"].cpu().numpy(), out["melspec_lens"].cpu().numpy()
        if prosody:
            pro = {k: v.cpu().numpy() for k, v in pe(wave_dev, lens_host).items()}
        for b, name in enumerate(ids):
            fields = {"melspec": np.ascontiguousarray(mel[b, :int(mel_lens[b])].T, dtype=np.float32)}
            if prosody:
                n = min(int(pro["frames"][b]), int(mel_lens[b]))
                fields.update(f0=np.ascontiguousarray(pro["f0"][b, :n], dtype=np.float32),
                              voiced=np.ascontiguousarray(pro["voiced"][b, :n], dtype=np.bool_),
                              energy=np.ascontiguousarray(pro["energy"][b, :n], dtype=np.float32))
            if sequences is not None:
                src = os.path.join(sequences, name + ".npz")
                if not os.path.isfile(src):
                    log(f"skipped {name}: no {src}")
                    continue
                with np.load(src, allow_pickle=True) as d:
                    fields.update({k: d[k] for k in ("transcript", "phoneme", "sequence")})
            np.savez(os.path.join(out_dir, name + ".npz"), **fields)
            written += 1
    log(f"{written} files -> {out_dir}")
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sequences", default=None)
    ap.add_argument("--stats", default="stats.json")
    ap.add_argument("--resample", action="store_true", help="bring recordings at another rate to the config's on the device")
    ap.add_argument("--prosody", action="store_true", help="add f0, voiced and energy per frame (audio.PitchEnergy) to each file")
    args = ap.parse_args(argv)
    import yaml
    with open(args.config, "r") as f:
        config = yaml.safe_load(f)
    run(config, batch=args.batch, sequences=args.sequences, stats_path=args.stats, resample=args.resample, prosody=args.prosody)


if __name__ == "__main__":
    main()
