"""Host side of ragged WAVES: per-row sample counts through resample and the codec encoders (include/vbx.h "ragged waves").
`lens` [B] of a padded wave batch [B, T] says row b holds lens[b] real samples; every front end then makes row b the row it would be
alone -- bit for bit up to its own frame count, exactly 0.0 past it -- and codec.frame_lens(lens) is what the latent-side `lens=`
machinery (train_lens.py, sample_lens.py) takes from there; a wav2vec= that serves lengths (HubertWithKmeans) gives the token ids of
every row alone and their counts, token_lens=.  Nothing here launches a kernel.

A list / tuple or a CPU tensor is validated on the host (ValueError naming the row); a device tensor is clamped into the same range
on the device without a host synchronisation: an unchecked length never reaches a kernel."""
import inspect
import math

import torch


def map_lens(lens, fn):
    """fn (integer arithmetic with +, *, //) over lengths given as a list / tuple, a CPU tensor or a device tensor; the same kind
    comes back (a tensor keeps its dtype and device, the arithmetic runs in int64)"""
    if torch.is_tensor(lens):
        if lens.dtype == torch.bool or lens.is_floating_point() or lens.is_complex():
            raise ValueError(f"lens must be an int tensor, got dtype {lens.dtype}")
        return fn(lens.detach().to(torch.int64)).to(lens.dtype)
    vals = list(lens)
    if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
        raise ValueError(f"lens must hold ints, got {vals!r}")
    return [int(fn(v)) for v in vals]


def device_lens(lens, B, T, min_len, device, who, name="lens"):
    """lens -> int32 [B] on `device`, min_len <= len_b <= T: what a *_lens kernel takes.  Host values are checked (ValueError naming
    the row), a device tensor is clamped.  name: what the messages call the lengths."""
    if torch.is_tensor(lens):
        if lens.dtype == torch.bool or lens.is_floating_point() or lens.is_complex():
            raise ValueError(f"{who}: {name} must be an int tensor, got dtype {lens.dtype}")
        if lens.ndim != 1 or lens.shape[0] != B:
            raise ValueError(f"{who}: {name} must have one entry per batch row: shape {tuple(lens.shape)} for a batch of {B}")
        if lens.device.type != "cpu":
            return lens.detach().to(device).clamp(min_len, T).to(torch.int32).contiguous()
        vals = lens.detach().to(torch.int64).tolist()
    else:
        vals = list(lens)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
            raise ValueError(f"{who}: {name} must hold ints, got {vals!r}")
        if len(vals) != B:
            raise ValueError(f"{who}: {name} must have one entry per batch row: {len(vals)} for a batch of {B}")
    for b, v in enumerate(vals):
        if v < min_len or v > T:
            raise ValueError(f"{who}: {name}[{b}] = {v} is outside {min_len} .. T = {T}")
    return torch.tensor(vals, dtype=torch.int32).to(device)


def zero_dead_frames(latents, frame_lens):
    """latents [B, F, D] with rows past frame_lens[b] (int tensor [B] on the same device) set to exactly 0.0, in place"""
    dead = torch.arange(latents.shape[1], device=latents.device)[None, :] >= frame_lens[:, None]
    return latents.masked_fill_(dead[:, :, None], 0.0)


def resample_lens(lens, orig_freq, new_freq):
    """the per-row output lengths of resample(waveform, orig_freq, new_freq, lens=lens): ceil(new * l / orig) with the rates reduced
    by their gcd; equal rates give the lengths back.  A list, a CPU tensor or a device tensor; the same kind comes back."""
    if not (int(orig_freq) == orig_freq and int(new_freq) == new_freq) or orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"need integral orig_freq > 0 and new_freq > 0 (got {orig_freq}, {new_freq})")
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    return map_lens(lens, lambda l: (l * new + (orig - 1)) // orig)


def codec_lacks(codec):
    """what `codec` lacks to serve wave_lens, as text, or None: frame_lens(sample_lens) and encode(audio, lens=)"""
    missing = []
    if not callable(getattr(codec, "frame_lens", None)):
        missing.append("frame_lens(sample_lens)")
    try:
        has = "lens" in inspect.signature(codec.encode).parameters
    except (TypeError, ValueError, AttributeError):
        has = False
    if not has:
        missing.append("`lens` in encode's signature")
    return " and ".join(missing) if missing else None


def wav2vec_lacks(w2v):
    """what `w2v` lacks to make token ids under wave_lens, as text, or None: `lens` in its call signature (forward(wave, lens=) of a
    module, __call__(wave, lens=) of any other object) and frame_lens(sample_lens)"""
    missing = []
    try:
        fn = w2v.forward if isinstance(w2v, torch.nn.Module) else w2v
        has = "lens" in inspect.signature(fn).parameters
    except (TypeError, ValueError, AttributeError):
        has = False
    if not has:
        missing.append("`lens` in its call signature")
    if not callable(getattr(w2v, "frame_lens", None)):
        missing.append("frame_lens(sample_lens)")
    return " and ".join(missing) if missing else None


def refuse_token_lens(token_lens, has_lens, token_ids, phoneme_ids, who, name="token_lens"):
    """every refusal of token_lens= (per-row token counts: row b's ids are resized to its own frames), before anything is launched"""
    if token_lens is None:
        return
    if phoneme_ids is not None:
        raise ValueError(f"{who}: {name} with phoneme_ids -- phonemes are aligned to frames by durations, not resized; {name} goes with "
                         f"semantic_token_ids")
    if token_ids is None:
        raise ValueError(f"{who}: {name} counts the token ids of each row, and no token ids were given")
    if not has_lens:
        raise ValueError(f"{who}: {name} resizes row b's ids to row b's own frames, which only lens= (or wave_lens=) tells -- pass one of them")


def token_lens_device(token_lens, B, T, device, who, name="token_lens"):
    """token_lens -> int32 [B] on `device`, 1 <= T_b <= T: host values are checked (ValueError naming the row), a device tensor clamped"""
    return device_lens(token_lens, B, T, 1, device, who, name=name)


def refuse(wave_lens, x1, cond, lens, mask, codec, who, wav2vec_ids=False, what="x1", wav2vec=None):
    """every refusal of wave_lens=, before anything is launched.  wav2vec_ids: the token ids would come from a wav2vec= that cannot
    serve lengths (wav2vec_lacks; `wav2vec`, when given, is named with what it lacks)"""
    is_wave = lambda t: torch.is_tensor(t) and (t.ndim == 2 or (t.ndim == 3 and t.shape[1] == 1))
    if lens is not None or mask is not None:
        other = "lens" if lens is not None else "mask"
        raise ValueError(f"{who}: wave_lens and {other} both given -- wave_lens counts the samples of raw audio and becomes the frame "
                         f"lengths itself; pass one of them")
    if not is_wave(x1):
        got = f"{tuple(x1.shape)} holds latents" if torch.is_tensor(x1) else "is not a wave batch"
        raise ValueError(f"{who}: wave_lens counts samples of raw audio (batch, samples), and {what} {got} -- pass lens in frames")
    if codec is None:
        raise ValueError(f"{who}: wave_lens needs audio_enc_dec on the VoiceBox to encode the waves")
    lacks = codec_lacks(codec)
    if lacks:
        raise ValueError(f"{who}: wave_lens needs a codec that is the row alone under lengths; {type(codec).__name__} has no {lacks}")
    if wav2vec_ids:
        why = "its group norm runs over time, a padded row is not the row alone"
        if wav2vec is not None and wav2vec_lacks(wav2vec):
            why = f"a padded row must be the row alone: {type(wav2vec).__name__} has no {wav2vec_lacks(wav2vec)}"
        raise NotImplementedError(f"{who}: wave_lens with token ids from wav2vec= is not built ({why}) -- pass semantic_token_ids")
