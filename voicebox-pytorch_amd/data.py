"""AudioDataset: a folder of audio files as a dataset of mono fp32 waves [T] -- what VoiceBoxTrainer(dataset=...) of a codec model
takes (with mask_wave_padding=True the collate function's lengths reach the step as wave_lens=).  Host only.

The shape is the reference's (voicebox_pytorch/data.py: a recursive glob over `folder`, the same two asserts, __getitem__ returning
the wave without its channel dimension).  ONE DIFFERENCE: the reference's default audio_extension is ".flac", which it decodes with
torchaudio; torchaudio is not a dependency here, and without it only PCM ".wav" (the stdlib `wave` module), ".pt" and ".npy" files
can be read -- so the default is ".wav".  With torchaudio installed every format it loads is served, ".flac" included."""
import wave as _wave
from pathlib import Path

import torch
from torch.utils.data import Dataset


def _torchaudio():
    try:
        import torchaudio

        return torchaudio
    except Exception:  # not installed, or installed against another torch
        return None


def read_pcm_wav(path):
    """a PCM .wav of 8 (unsigned), 16, 24 or 32 bits -> (fp32 [channels, T] in [-1, 1), sampling rate): int / 2^(bits - 1), the
    8-bit format centred at 128"""
    with _wave.open(str(path), "rb") as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(n)
    if width == 1:
        x = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(torch.float32).sub_(128.0).div_(128.0)
    elif width == 2:
        x = torch.frombuffer(bytearray(raw), dtype=torch.int16).to(torch.float32).div_(32768.0)
    elif width == 3:
        b = torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(-1, 3).to(torch.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).to(torch.float32).div_(8388608.0)
    elif width == 4:
        x = torch.frombuffer(bytearray(raw), dtype=torch.int32).to(torch.float64).div_(2147483648.0).to(torch.float32)
    else:
        raise ValueError(f"{path}: {8 * width}-bit PCM is not served (8, 16, 24 and 32 bits are)")
    return x.reshape(-1, ch).t().contiguous(), rate


class AudioDataset(Dataset):
    def __init__(self, folder, audio_extension=".wav"):
        super().__init__()
        path = Path(folder)
        assert path.exists(), 'folder does not exist'
        self.audio_extension = audio_extension
        files = sorted(path.glob(f'**/*{audio_extension}'))
        assert len(files) > 0, 'no files found'
        self.files = files

    def __len__(self):
        return len(self.files)

    def _load(self, file):
        """fp32 [channels, T] or [T]"""
        ext = file.suffix.lower()
        if ext == ".pt":
            return torch.as_tensor(torch.load(str(file), map_location="cpu"))
        if ext == ".npy":
            import numpy as np

            return torch.from_numpy(np.load(str(file)))
        ta = _torchaudio()
        if ta is not None:
            return ta.load(str(file))[0]
        if ext == ".wav":
            try:
                return read_pcm_wav(file)[0]
            except _wave.Error as e:
                raise RuntimeError(f"{file}: not a PCM .wav the stdlib `wave` module reads ({e}); torchaudio is not installed") from None
        raise RuntimeError(f"{file}: no decoder for '{ext}' files -- torchaudio is not installed, and without it only PCM .wav, .pt and "
                           f".npy are read")

    def __getitem__(self, idx):
        file = self.files[idx]
        w = self._load(file)
        if w.ndim == 2 and w.shape[0] == 1:
            w = w[0]
        if w.ndim != 1:
            raise RuntimeError(f"{file}: {tuple(w.shape)} is not a mono wave (channels, samples) = (1, T) -- mix it down first")
        return w.to(torch.float32)
