"""A weight-free test codec for the audio_enc_dec interface (tests only): `hop` samples per frame, one fixed [hop, latent_dim]
matrix.  encode: [B, T] -> [B, T // hop, latent_dim]; decode: the pseudo-inverse, flattened back to a wave.  Duck-typed on
purpose: it does not inherit from AudioEncoderDecoder."""
import torch
from torch import nn


class ToyCodec(nn.Module):
    def __init__(self, latent_dim, hop=16, sampling_rate=24000):
        super().__init__()
        self.hop = hop
        self._latent_dim = latent_dim
        self._sampling_rate = sampling_rate
        w = torch.randn(hop, latent_dim, generator=torch.Generator().manual_seed(3)) * hop ** -0.5
        self.register_buffer("w", w, persistent=False)
        self.register_buffer("w_pinv", torch.linalg.pinv(w.double()).float(), persistent=False)

    @property
    def latent_dim(self):
        return self._latent_dim

    @property
    def sampling_rate(self):
        return self._sampling_rate

    @property
    def downsample_factor(self):
        return self.hop

    def encode(self, audio):
        if audio.ndim == 3:
            audio = audio[:, 0]
        b, t = audio.shape
        frames = audio[:, :t // self.hop * self.hop].reshape(b, t // self.hop, self.hop)
        return frames.float() @ self.w.to(frames.device)

    def decode(self, latents):
        return (latents @ self.w_pinv.to(latents.device)).reshape(latents.shape[0], -1)

    def decode_to_codes(self, latents):
        return latents.argmax(dim=-1)
