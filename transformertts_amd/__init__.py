"""transformertts_amd -- MI355X-native (gfx950) teacher-forced Transformer-TTS forward/backward.

Drop-in for the reference's `model` package surface:
    from transformertts_amd.model import TransformerTTS
Host code is Python on PyTorch-ROCm (memory, streams, autograd graph, torch.distributed); every
arithmetic step of the path runs in hand-written HIP kernels behind the C ABI of include/ttts_hip.h.
"""
__all__ = ["model", "ops", "extract_durations", "teacher_durations", "AttentionWindow", "dtw_distance", "mel_cepstra",
           "evaluate_synthesis", "MelFrontEnd", "mel_filterbank", "read_wav", "normalize", "denormalize", "Vocoder", "write_wav_pcm16",
           "Resampler", "resample_table", "read_wav_native", "PitchEnergy", "phoneme_average", "length_regulate", "LengthRegulator",
           "durations_from_log", "variance_embed", "VarianceEmbedding", "variance_bins", "VarianceLoss", "VariancePredictor",
           "VarianceAdaptor", "ragged_conv_norm", "RaggedConvNorm", "KernelVariancePredictor", "ragged_conv_ffn", "ConvFeedForward",
           "FFTBlock", "FFTStack", "FastSpeech2Student", "mel_loss", "FastSpeech2Loss", "StudentTrainStep", "distillation_targets",
           "synth_student_batch", "HiFiGANConfig", "HiFiGANGenerator", "fold_weight_norm", "transposed_as_conv", "ragged_dilated_conv",
           "load_hifigan"]


def __getattr__(name):          # the two calls of alignment.py, imported (and torch with them) when first asked for
    if name in ("extract_durations", "teacher_durations"):
        from . import alignment
        return getattr(alignment, name)
    if name == "AttentionWindow":   # the window of Synthesizer.synthesize(window=...)
        from . import synthesis
        return synthesis.AttentionWindow
    if name in ("dtw_distance", "mel_cepstra", "evaluate_synthesis"):   # free-running validation (metrics.py)
        from . import metrics
        return getattr(metrics, name)
    if name in ("MelFrontEnd", "mel_filterbank", "read_wav", "normalize", "denormalize"):   # log-mel front end (audio.py)
        from . import audio
        return getattr(audio, name)
    if name in ("Vocoder", "write_wav_pcm16"):   # Griffin-Lim vocoder (audio.py)
        from . import audio
        return getattr(audio, name)
    if name in ("Resampler", "resample_table", "read_wav_native"):   # band-limited resampler (audio.py)
        from . import audio
        return getattr(audio, name)
    if name in ("PitchEnergy", "phoneme_average"):   # frame pitch and energy, phoneme means (audio.py)
        from . import audio
        return getattr(audio, name)
    if name in ("length_regulate", "LengthRegulator", "durations_from_log", "variance_embed", "VarianceEmbedding", "variance_bins",
                "VarianceLoss", "VariancePredictor", "VarianceAdaptor"):   # variance adaptor of a FastSpeech-2 student (variance.py)
        from . import variance
        return getattr(variance, name)
    if name in ("ragged_conv_norm", "RaggedConvNorm", "KernelVariancePredictor"):   # the predictor on the kernels (predictor.py)
        from . import predictor
        return getattr(predictor, name)
    if name in ("ragged_conv_ffn", "ConvFeedForward", "FFTBlock", "FFTStack", "FastSpeech2Student"):   # FFT blocks, the student (fft.py)
        from . import fft
        return getattr(fft, name)
    if name in ("mel_loss", "FastSpeech2Loss", "StudentTrainStep", "distillation_targets"):   # training the student (student.py)
        from . import student
        return getattr(student, name)
    if name == "synth_student_batch":   # a synthetic batch with the student's seven keys (workload.py)
        from . import workload
        return workload.synth_student_batch
    if name in ("HiFiGANConfig", "HiFiGANGenerator", "fold_weight_norm", "transposed_as_conv", "ragged_dilated_conv",
                "load_hifigan"):   # the HiFi-GAN generator on the kernels (hifigan.py)
        from . import hifigan
        return getattr(hifigan, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
