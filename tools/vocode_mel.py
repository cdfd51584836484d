#!/usr/bin/env python3
"""A `.npz` written by tools/preprocess_mel.py (or a synthesised mel saved the same way) -> a PCM16 `.wav`, through `Vocoder`
(csrc/vocoder.hip): pseudo-inverse mel basis, then fast Griffin-Lim.

    python tools/vocode_mel.py --config config.yaml --npz FILE.npz [--stats stats.json] --out FILE.wav [--n-iter 32] [--out-rate R]
                               [--hifigan CKPT --hifigan-config JSON]

`melspec` in the file is (n_mels, T) fp32.  With `config['audio']['normalize_mel']` the file holds normalised values and
`--stats` (the `mean` / `std` file of preprocess_mel.py) is needed to undo that.  The wave has (T - 1) * hop_length samples at
`config['audio']['sample_rate']`, or with `--out-rate R` is resampled on the device to R Hz (`audio.Resampler`,
csrc/resample.hip) before it is written; a mel too short to vocode ((T - 1) * hop_length <= n_fft/2) is refused.
With `--hifigan CKPT --hifigan-config JSON` the wave comes from a HiFi-GAN generator instead (`load_hifigan`, csrc/hifigan.hip): CKPT
is a generator checkpoint as `torch.load` reads it, JSON its `config.json`; the wave then has T * hop_length samples, any T >= 1 is
taken, `--n-iter` is not used, and the generator's hop and mel count must be the config's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from transformertts_amd import audio  # noqa: E402


def make_vocoder(audio_config, mean=None, std=None, **kw):
    return audio.Vocoder(audio_config, mean=mean, std=std, **kw)


def make_hifigan(ckpt, config_json, mean=None, std=None):
    from transformertts_amd import hifigan
    return hifigan.load_hifigan(ckpt, hifigan.HiFiGANConfig.from_json(config_json), mean=mean, std=std)


def make_resampler(orig_rate, new_rate):
    return audio.Resampler(orig_rate, new_rate)


def run(config, npz_path, out_path, stats_path=None, make_vocoder=make_vocoder, log=print, out_rate=None, hifigan=None,
        hifigan_config=None, make_hifigan=make_hifigan, **kw):
    a = config["audio"]
    mean = std = None
    if a.get("normalize_mel"):
        if stats_path is None:
            raise ValueError("config['audio']['normalize_mel'] is set: --stats (the mean / std file of preprocess_mel.py) is needed")
        with open(stats_path, "r", encoding="utf-8") as f:
            stats = json.load(f)
        mean, std = float(stats["mean"]), float(stats["std"])
    with np.load(npz_path, allow_pickle=True) as d:
        mel = np.asarray(d["melspec"], dtype=np.float32)
    n_mels, hop, n_fft = int(a["n_mels"]), int(a["hop_length"]), int(a["n_fft"])
    if mel.ndim != 2 or mel.shape[0] != n_mels:
        raise ValueError(f"{npz_path}: melspec must be ({n_mels}, T), got {mel.shape}")
    T = mel.shape[1]
    if (hifigan is None) != (hifigan_config is None):
        raise ValueError("--hifigan and --hifigan-config go together")
    if hifigan is not None:
        if T < 1:
            raise ValueError(f"{npz_path}: no frames to vocode")
        voc = make_hifigan(hifigan, hifigan_config, mean=mean, std=std)
        if voc.config.n_mels != n_mels or voc.hop != hop:
            raise ValueError(f"{hifigan_config}: the generator takes {voc.config.n_mels} mels at a hop of {voc.hop}, the audio config has "
                             f"{n_mels} and {hop}")
    else:
        if (T - 1) * hop <= n_fft // 2:
            raise ValueError(f"{npz_path}: {T} frames are too few to vocode ((T - 1) * hop_length must exceed n_fft/2 = {n_fft // 2})")
        voc = make_vocoder(a, mean=mean, std=std, **kw)
    out = voc(torch.from_numpy(np.ascontiguousarray(mel.T))[None].to(voc.device), torch.tensor([T], dtype=torch.int64))
    rate = int(a["sample_rate"])
    if out_rate is not None and int(out_rate) != rate:
        out = make_resampler(rate, int(out_rate))(out["wave"], out["wave_lens"])
        rate = int(out_rate)
    n = int(out["wave_lens"][0])
    wave = out["wave"][0, :n].cpu().numpy()
    peak = float(np.abs(wave).max()) if n else 0.0
    if peak >= 1.0:                                                   # PCM16 clips at full scale
        log(f"peak {peak:.3f}: scaled to 0.99")
        wave = wave * (0.99 / peak)
    audio.write_wav_pcm16(out_path, wave, rate)
    log(f"{n} samples ({n / float(rate):.2f} s) -> {out_path}")
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--npz", required=True)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--out-rate", type=int, default=None, help="write the wave at this rate instead of the config's")
    ap.add_argument("--hifigan", default=None, help="a HiFi-GAN generator checkpoint: vocode with it instead of Griffin-Lim")
    ap.add_argument("--hifigan-config", default=None, help="the checkpoint's config.json")
    args = ap.parse_args(argv)
    import yaml
    with open(args.config, "r") as f:
        config = yaml.safe_load(f)
    if args.hifigan is not None or args.hifigan_config is not None:
        run(config, args.npz, args.out, stats_path=args.stats, out_rate=args.out_rate, hifigan=args.hifigan,
            hifigan_config=args.hifigan_config)
        return
    run(config, args.npz, args.out, stats_path=args.stats, n_iter=args.n_iter, out_rate=args.out_rate)


if __name__ == "__main__":
    main()
