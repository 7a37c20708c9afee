"""voicebox-pytorch_amd: MI355X (gfx950) native hot path of lucidrains/voicebox-pytorch.

Public API mirrors the reference package (voicebox_pytorch/__init__.py:1-15) for the hot path:
VoiceBox, ConditionalFlowMatcherWrapper, Transformer, Attend, DurationPredictor (inference), VoiceBoxTrainer (latents or waves),
AudioEncoderDecoder / LogMelCodec (the codec interface, the log-mel encoder and its vocoder-free decode), griffin_lim (Griffin-Lim
phase recovery on the device), resample / Resample (sample-rate conversion on the device, in front of a codec), VocosDecoder (the
Vocos neural vocoder's decoder on the device; weights are the user's, from a local checkpoint), VocosEncodecDecoder (its
EnCodec-conditioned variant as published: AdaLayerNorm tables, n_fft 1280, padding="same"), ResidualVQ / EncodecVocoCodec
(EnCodec's residual vector quantizer on the device and the reference's EncodecVoco around it: codes in and out), SEANetEncoder
(EnCodec's encoder on the device: waves into that codec; weights are the user's, from a local checkpoint), SEANetDecoder (EnCodec's
decoder on the device: that codec's latents back into waves, from the same local checkpoint), CausalSEANetEncoder /
CausalSEANetDecoder (the same two in EnCodec's causal form, which the published 24 kHz model needs), maximum_path / forward_sum_loss /
ForwardSumLoss (monotonic alignment search and the forward-sum loss on the device: what an aligner is trained with), Aligner /
aligner_attention (the alignment network itself, forward and backward on the device: phonemes and mels into durations),
HiFiGANGenerator (HiFi-GAN's generator on the device: mels into waves, a `vocoder=` of LogMelCodec; weights are the user's, from a
local checkpoint), BigVGANGenerator (BigVGAN's generator on the device, its anti-aliased snake activations in HIP: the same call
shape; a local checkpoint and its config.json), HiFiGANMelCodec / mel_spectrogram (the mel front end those two generators were
trained on -- Slaney filters, magnitude, ln, center=False -- in one kernel: the codec published HiFi-GAN / BigVGAN weights want),
HubertWithKmeans (HuBERT base up to one encoder layer plus a k-means codebook on the device: waves into semantic token ids, the
`wav2vec=` of ConditionalFlowMatcherWrapper; weights are the user's, from local files), HubertLargeWithKmeans / normalize_wave (the
same for HuBERT large -- per-layer convolution norms, the pre-LN encoder: hubert-large-ll60k -- and the zero-mean unit-variance wave
that model was trained on), KMeans / kmeans_plusplus (fitting that
codebook on the device from features: minibatch and Lloyd steps, D^2 sampling; HubertWithKmeans.fit_kmeans), AudioDataset (a folder of audio
files as a dataset of waves) and resample_lens (the length arithmetic of resample(lens=): ragged wave batches, `wave_lens=`).
"""
from . import _lib  # noqa: F401

__all__ = ["_lib"]
try:  # model classes need torch; keep `_lib` importable on its own
    from .masks import mask_from_frac_lengths, mask_from_start_end_indices, prob_mask_like, reduce_masks_with_and  # noqa: F401
    from .model import VoiceBox, ConditionalFlowMatcherWrapper, Transformer, Attend  # noqa: F401
    from .trainer import VoiceBoxTrainer  # noqa: F401
    from .duration import DurationPredictor  # noqa: F401
    from .codec import AudioEncoderDecoder, LogMelCodec, griffin_lim, resample, Resample, ResidualVQ, EncodecVocoCodec  # noqa: F401
    from .codec import HiFiGANMelCodec, mel_spectrogram  # noqa: F401
    from .codec import resample_lens  # noqa: F401  (the per-row lengths behind resample(lens=): ragged waves, wave_lens.py)
    from .data import AudioDataset  # noqa: F401
    from .vocos import VocosDecoder, VocosEncodecDecoder  # noqa: F401
    from .seanet import CausalSEANetDecoder, CausalSEANetEncoder, SEANetDecoder, SEANetEncoder  # noqa: F401
    from .hifigan import HiFiGANGenerator  # noqa: F401
    from .bigvgan import BigVGANGenerator  # noqa: F401
    from .hubert import HubertWithKmeans, HubertLargeWithKmeans, normalize_wave  # noqa: F401
    from .kmeans import KMeans, kmeans_plusplus  # noqa: F401
    from .align import maximum_path, forward_sum_loss, ForwardSumLoss, Aligner, aligner_attention  # noqa: F401
    from .engine import precise_mode, set_precise, precise_enabled  # noqa: F401
    from .dp import ema_decay_at  # noqa: F401  (the decay schedule of dp.TrainStep(ema_decay=))
    from . import lora  # noqa: F401  (VoiceBox.add_lora / lora_state_dict / load_lora_state_dict / merge_lora / detach_lora)

    __all__ += ["VoiceBox", "ConditionalFlowMatcherWrapper", "Transformer", "Attend", "VoiceBoxTrainer", "DurationPredictor", "mask_from_frac_lengths",
                "mask_from_start_end_indices", "prob_mask_like", "reduce_masks_with_and", "precise_mode", "set_precise", "precise_enabled",
                "AudioEncoderDecoder", "LogMelCodec", "griffin_lim", "resample", "Resample", "VocosDecoder", "VocosEncodecDecoder", "ResidualVQ", "EncodecVocoCodec", "SEANetEncoder", "SEANetDecoder",
                "CausalSEANetEncoder", "CausalSEANetDecoder", "HiFiGANGenerator", "BigVGANGenerator", "HubertWithKmeans", "HiFiGANMelCodec", "mel_spectrogram",
                "maximum_path", "forward_sum_loss", "ForwardSumLoss", "Aligner", "aligner_attention", "lora", "ema_decay_at", "resample_lens",
                "AudioDataset", "KMeans", "kmeans_plusplus", "HubertLargeWithKmeans", "normalize_wave"]
except ModuleNotFoundError as _e:  # pragma: no cover - only while the package is being bootstrapped
    if "masks" not in str(_e) and "model" not in str(_e):
        raise
