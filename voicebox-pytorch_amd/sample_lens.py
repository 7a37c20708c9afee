"""Host side of sample(lens=, length_bucket=) (model.ConditionalFlowMatcherWrapper.sample): validation, bucket arithmetic, the padding
up to a bucket, the per-row decode, and the length regulator (csrc/duration.hip vbx_length_regulate) with its torch restatement.
Nothing here launches a forward; the masked samplers are in solver.py."""
import torch

from . import _lib


def validate_lens(lens, B, N):
    """lens: a list / tuple or an int tensor [B] on any device -> int32 CPU tensor [B] (the one host read), 1 <= len_b <= N."""
    if isinstance(lens, torch.Tensor):
        if lens.dtype in (torch.bool,) or lens.is_floating_point() or lens.is_complex():
            raise ValueError(f"lens must be an int tensor, got dtype {lens.dtype}")
        t = lens.detach().to("cpu", torch.int64)
    else:
        vals = list(lens)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
            raise ValueError(f"lens must hold ints, got {vals!r}")
        t = torch.tensor(vals, dtype=torch.int64)
    if t.ndim != 1 or t.shape[0] != B:
        raise ValueError(f"lens must have one entry per batch row: shape {tuple(t.shape)} for a batch of {B}")
    vals = t.tolist()
    for b, v in enumerate(vals):
        if v == 0:
            raise ValueError(f"lens[{b}] = 0: a row without frames has no sample -- leave it out of the batch")
        if v < 0 or v > N:
            raise ValueError(f"lens[{b}] = {v} is outside 1 .. N = {N}")
    return t.to(torch.int32)


def bucketed(N, length_bucket):
    """the frame count the sampler runs at: N rounded up to a multiple of length_bucket (None: N itself)"""
    if length_bucket is None:
        return N
    if isinstance(length_bucket, bool) or not isinstance(length_bucket, int) or length_bucket < 1:
        raise ValueError(f"length_bucket must be an int >= 1, got {length_bucket!r}")
    return -(-N // length_bucket) * length_bucket


def pad_frames(Nb, cond, y0, cond_mask, cond_token_ids):
    """cond / y0 [B, N, D], cond_mask [B, N] or None, ids [B, N] or None, extended to Nb frames: zeros, "masked", id 0"""
    n = Nb - cond.shape[1]
    pad3 = lambda x: torch.nn.functional.pad(x, (0, 0, 0, n))
    if cond_mask is not None:
        cond_mask = torch.nn.functional.pad(cond_mask.to(torch.bool), (0, n), value=True)
    if cond_token_ids is not None:
        cond_token_ids = torch.nn.functional.pad(cond_token_ids, (0, n), value=0)
    return pad3(cond), pad3(y0), cond_mask, cond_token_ids


def mask_codes(codes, lens):
    """codes [B, N, ...] of the padded latents: -1 from frame len_b on"""
    dead = torch.arange(codes.shape[1], device=codes.device)[None] >= lens.to(codes.device)[:, None]
    return codes.masked_fill(dead.reshape(dead.shape + (1,) * (codes.ndim - 2)), -1)


def decode_rows(codec, latents, lens):
    """Row b of the result is codec.decode(latents[b:b+1, :len_b]): rows of equal length are decoded together (the decoders are
    row-stable), the waves zero-filled to the longest.  -> (wave [B, ..., T], samples per row int64 CPU [B])"""
    vals = lens.tolist()
    waves, out_lens = [None] * len(vals), torch.zeros(len(vals), dtype=torch.int64)
    for L in sorted(set(vals)):
        rows = [b for b, v in enumerate(vals) if v == L]
        w = codec.decode(latents[rows, :L].contiguous())
        for i, b in enumerate(rows):
            waves[b] = w[i]
            out_lens[b] = w.shape[-1]
    T = int(out_lens.max())
    return torch.stack([torch.nn.functional.pad(w, (0, T - w.shape[-1])) for w in waves]), out_lens


def length_regulate_restated(phoneme_ids, durations):
    """What vbx_length_regulate computes, in torch (any device): phoneme i of row b with id != -1 owns int(clamp(duration, min=1))
    frames, a -1 padding phoneme none -> (aligned int64 [B, max_b len_b]: the id over its run, 0 from len_b on; lens int64 [B]).
    On a row without padding phonemes this is DurationPredictor.align_phoneme_ids_with_durations; on a row with them that helper
    also gives every padding phoneme its clamped duration in frames of id -1."""
    ids = phoneme_ids.to(torch.int64)
    reps = torch.where(ids != -1, durations.float().clamp(min=1).to(torch.int64), torch.zeros_like(ids))
    end = reps.cumsum(-1)
    lens = end[:, -1]
    pos = torch.arange(int(lens.max()), device=ids.device)
    owner = (pos[None, None] >= (end - reps)[..., None]) & (pos[None, None] < end[..., None])  # [B, K, Nmax]: at most one per column
    return (ids[..., None] * owner).sum(1), lens


def durations_lens(phoneme_ids, durations):
    """The length regulator on the device: (aligned ids int64 [B, Nmax], lens int32 CPU [B]).  Two launches of vbx_length_regulate
    around the one host read that sizes the result (generate_mask_from_repeats pays the same read); no [B, K, Nmax] mask."""
    ids = phoneme_ids.to(torch.int64).contiguous()
    dur = durations.to(torch.float32).contiguous()
    B, K = ids.shape
    lens_dev = torch.empty(B, dtype=torch.int32, device=ids.device)
    st = _lib.current_stream()
    _lib.call("vbx_length_regulate", ids, dur, None, lens_dev, B, K, 0, st)
    lens = lens_dev.cpu()
    Nmax = int(lens.max())
    if Nmax < 1:
        raise ValueError("lens='durations': every phoneme id is -1, there is nothing to sample")
    aligned = torch.empty(B, Nmax, dtype=torch.int64, device=ids.device)
    _lib.call("vbx_length_regulate", ids, dur, aligned, lens_dev, B, K, Nmax, st)
    return aligned, lens
