"""Host side of training on ragged batches by lengths (lens=): the refusals and their messages before any device call, the mask /
key_lens construction, and the trainer's collate function under mask_padding.  The device side is tests/test_train_lens_gpu.py."""
import pytest
import torch
from torch.nn.utils.rnn import pad_sequence


def _wrapper():
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=5, depth=2, dim_head=64, heads=2, condition_on_text=False)
    return vbx, vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def test_wrapper_refusals_and_messages():
    """lens with mask, lens with raw audio, out-of-range entries (the row is named, as sample(lens=) names it), wrong shape and dtype:
    ValueError on a CPU wrapper, i.e. before anything could be launched"""
    _, vb, w = _wrapper()
    x1 = torch.randn(3, 40, 64)
    with pytest.raises(ValueError, match=r"lens and mask both given.*pass one of them"):
        w(x1, lens=[40, 7, 1], mask=torch.ones(3, 40, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"raw audio.*encode first.*or pass mask"):
        w(torch.randn(3, 16000), lens=[40, 7, 1])
    with pytest.raises(ValueError, match=r"raw audio"):
        w(torch.randn(3, 1, 16000), lens=torch.tensor([40, 7, 1]))
    with pytest.raises(ValueError, match=r"lens\[1\] = 41 is outside 1 \.\. N = 40"):
        w(x1, lens=[40, 41, 1])
    with pytest.raises(ValueError, match=r"lens\[2\] = -1"):
        w(x1, lens=torch.tensor([40, 7, -1]))
    with pytest.raises(ValueError, match=r"lens\[0\] = 0"):
        w(x1, lens=[0, 7, 1])
    with pytest.raises(ValueError, match="one entry per batch row"):
        w(x1, lens=[40, 7])
    with pytest.raises(ValueError, match="one entry per batch row"):
        w(x1, lens=torch.ones(3, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="int tensor"):
        w(x1, lens=torch.tensor([40., 7., 1.]))
    with pytest.raises(ValueError, match=r"self_attn_lens and self_attn_mask both given"):
        vb(x1, times=torch.rand(3), cond_token_ids=None, target=x1, self_attn_lens=[40, 7, 1], self_attn_mask=torch.ones(3, 40, dtype=torch.bool))


def test_train_step_refusals_come_before_the_device():
    """TrainStep._forward_backward refuses the same combinations first thing (the step object itself needs a device: only the checks
    it runs are exercised here)"""
    from voicebox_pytorch_amd import train_lens

    with pytest.raises(ValueError, match=r"TrainStep: lens and mask both given"):
        train_lens.refuse_with_mask([1], torch.ones(1, 4, dtype=torch.bool), "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: lens counts frames, and x1 is raw audio"):
        train_lens.refuse_raw_audio([1], torch.randn(1, 800), "TrainStep")
    train_lens.refuse_with_mask(None, torch.ones(1, 4, dtype=torch.bool), "TrainStep")
    train_lens.refuse_raw_audio(None, torch.randn(1, 800), "TrainStep")
    train_lens.refuse_raw_audio([4], torch.randn(1, 4, 64), "TrainStep")


@pytest.mark.parametrize("length_bucket", [0, 64])
def test_mask_and_key_lens_construction(length_bucket):
    """frame_lens / prefix_mask / key_lens against arange < lens, from a list and from a tensor; with a length bucket the frames
    added behind N are False in the padded mask and key_lens = R + lens is what it was"""
    from voicebox_pytorch_amd import train_lens

    B, N, R = 4, 200, 16
    vals = [200, 1, 113, 64]
    for src in (vals, torch.tensor(vals), torch.tensor(vals, dtype=torch.int32)):
        lens = train_lens.frame_lens(src, B, N, torch.device("cpu"))
        assert lens.dtype == torch.int32 and lens.tolist() == vals
        mask = train_lens.prefix_mask(lens, N)
        want = torch.arange(N)[None] < torch.tensor(vals)[:, None]
        assert mask.dtype == torch.bool and torch.equal(mask, want) and mask.sum(1).tolist() == vals
        kl = train_lens.key_lens(lens, R)
        assert kl.dtype == torch.int32 and kl.is_contiguous() and kl.tolist() == [R + v for v in vals]
        if length_bucket:
            Nb = -(-N // length_bucket) * length_bucket
            padded = torch.nn.functional.pad(mask, (0, Nb - N), value=False)  # TrainStep's padm
            assert Nb == 256 and torch.equal(padded, torch.arange(Nb)[None] < torch.tensor(vals)[:, None])
            assert torch.equal(train_lens.key_lens(lens, R), kl) and int(kl.max()) <= R + N


def test_collate_returns_the_true_lengths_under_mask_padding():
    """_collate(with_lens=True): the padded columns as before, then the items' lengths before pad_sequence; with_lens=False (the
    default, mask_padding=False) returns exactly what it returns today"""
    from voicebox_pytorch_amd.trainer import VoiceBoxTrainer, _collate

    gen = torch.Generator().manual_seed(0)
    items = [torch.randn(n, 8, generator=gen) for n in (5, 9, 1, 7)]
    want = pad_sequence(items, batch_first=True)
    plain = _collate(True)(items)
    assert isinstance(plain, tuple) and len(plain) == 1 and torch.equal(plain[0], want)
    assert torch.equal(_collate(True, with_lens=False)(items)[0], want) and len(_collate(True, False)(items)) == 1
    x, lens = _collate(True, with_lens=True)(items)
    assert torch.equal(x, want) and lens.dtype == torch.int64 and lens.tolist() == [5, 9, 1, 7]
    # (latents, ids) items: the lengths are those of the first column
    ids = [torch.arange(n + 2) for n in (5, 9, 1, 7)]
    pairs = list(zip(items, ids))
    x2, i2 = _collate(True)(pairs)
    x3, i3, l3 = _collate(True, with_lens=True)(pairs)
    assert torch.equal(x2, x3) and torch.equal(i2, i3) and i2.shape == (4, 11) and l3.tolist() == [5, 9, 1, 7]
    # cropping instead of padding: every row has the cropped length
    xc, lc = _collate(False, with_lens=True)(items)
    assert xc.shape == (4, 1, 8) and lc.tolist() == [1, 1, 1, 1] and torch.equal(_collate(False)(items)[0], xc)
    # the trainer hands the lengths to the step as lens=, and refuses a dataset of waves at its first batch
    _, _, w = _wrapper()
    t = VoiceBoxTrainer.__new__(VoiceBoxTrainer)
    torch.nn.Module.__init__(t)
    t.cfm_wrapper, t.input_sampling_rate, t.mask_padding = w, None, True
    xb, kw = t._model_kwargs((x, lens))
    assert xb is x and set(kw) == {"lens"} and kw["lens"] is lens
    with pytest.raises(ValueError, match=r"mask_padding=True.*latents.*codec"):
        t._model_kwargs(_collate(True, with_lens=True)([torch.randn(n) for n in (800, 640)]))
    t.mask_padding = False
    assert t._model_kwargs((x,)) == (x, {})
