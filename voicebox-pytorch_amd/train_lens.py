"""Host side of training on ragged batches by lengths: wrapper(x1, lens=), VoiceBox.forward(self_attn_lens=), TrainStep.step(lens=).
lens [B] means exactly mask = arange(N)[None] < lens[:, None]; beside the mask bytes (which the convolutional position embedding, the
loss and the fallbacks keep reading) the attention forward and backward get key_lens = R + lens and do not walk the tiles past it
(include/vbx.h "attention backward with prefix lengths").  Nothing here launches a forward."""
import torch

from .sample_lens import validate_lens


def refuse_with_mask(lens, mask, who, lens_name="lens", mask_name="mask"):
    if lens is not None and mask is not None:
        raise ValueError(f"{who}: {lens_name} and {mask_name} both given -- {lens_name} means {mask_name} = arange(N) < {lens_name}[:, None]; "
                         f"pass one of them")


def refuse_raw_audio(lens, x1, who):
    """a wave batch: [B, samples] or [B, 1, samples] (model.is_probably_audio_from_shape)"""
    if lens is not None and torch.is_tensor(x1) and (x1.ndim == 2 or (x1.ndim == 3 and x1.shape[1] == 1)):
        raise ValueError(f"{who}: lens counts frames, and x1 is raw audio whose frame count is the codec's business -- encode first "
                         f"(wrapper.encode_raw_audio) and pass lens in frames, or pass mask, or pass wave_lens= (samples per row)")


def frame_lens(lens, B, N, device):
    """lens -> int32 [B] on `device`, 1 <= len_b <= N.  A list / tuple or a CPU tensor is validated on the host (ValueError naming the
    row, as sample(lens=)); a device tensor is clamped into 1 .. N on the device, with no host synchronisation: an unchecked length
    never reaches a kernel as an out-of-range bound."""
    if torch.is_tensor(lens) and lens.device.type != "cpu":
        if lens.dtype == torch.bool or lens.is_floating_point() or lens.is_complex():
            raise ValueError(f"lens must be an int tensor, got dtype {lens.dtype}")
        if lens.ndim != 1 or lens.shape[0] != B:
            raise ValueError(f"lens must have one entry per batch row: shape {tuple(lens.shape)} for a batch of {B}")
        return lens.detach().to(device).clamp(1, N).to(torch.int32)
    return validate_lens(lens, B, N).to(device)


def prefix_mask(lens, N):
    """bool [B, N] on the device of lens: frame n of row b is live iff n < lens[b]"""
    return torch.arange(N, device=lens.device)[None, :] < lens[:, None]


def key_lens(lens, R):
    """int32 [B]: the live rows of the attention sequence, R register rows in front of the frames.  Frames added behind N (TrainStep's
    length_bucket) lie past every length: key_lens does not change with them."""
    return (lens + R).to(torch.int32).contiguous()
