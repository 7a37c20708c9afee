"""Ragged waves on the device: per-row lengths through resample, the codec encoders, the wrapper, the train step and the sampler
(include/vbx.h "ragged waves", voicebox_pytorch_amd/wave_lens.py).  The contract is `lens` makes every row of a padded batch the row
it would be alone, so every comparison is torch.equal on the raw bits: row b up to its own output length against the plain entry on
x[b:b+1, :len_b], exactly 0.0 past it.  Every padded batch has NaN planted past each row's length (a kernel that reads there shows),
and every case runs from a list and from a device tensor of lengths, which must give the same bits.  tests/test_wave_lens_cpu.py
shows how far a kernel that ignored the lengths would move the last live frames."""
import pytest
import torch

import seanet_causal_ref as C
import seanet_ref as S

pytestmark = pytest.mark.gpu
dev = "cuda"


def _waves(lens, T, seed=0):
    """(padded [B, T] with NaN past each length, the rows alone)"""
    g = torch.Generator().manual_seed(4000 + seed)
    rows = [0.3 * torch.randn(l, generator=g) for l in lens]
    pad = torch.full((len(lens), T), float("nan"))
    for b, r in enumerate(rows):
        pad[b, :r.numel()] = r
    return pad.to(dev), [r.to(dev) for r in rows]


def _check_rows(encode, frame_lens, lens, T, seed=0, clamp=None):
    """encode(batch, lens) against encode(row) per row; list and device tensor of lengths; returns the batch result"""
    pad, rows = _waves(lens, T, seed)
    got = encode(pad, list(lens))
    got_dev = encode(pad, torch.tensor(lens, device=dev))
    assert torch.equal(got, got_dev), "a list and a device tensor of lengths give different bits"
    assert torch.equal(got, encode(pad, torch.tensor(lens))), "a CPU tensor of lengths gives different bits"
    assert torch.equal(got, encode(pad, list(lens))), "rerun differs"
    F = frame_lens(list(lens))
    assert got.shape[1] == max(F)
    for b, (r, f) in enumerate(zip(rows, F)):
        alone = encode(r[None], None)[0]
        assert alone.shape[0] == f, (b, alone.shape, f)
        assert torch.equal(got[b, :f], alone), (b, lens[b], f, float((got[b, :f] - alone).abs().max()))
        assert bool((got[b, f:] == 0).all()), (b, lens[b], "dead frames are not 0.0")
    if clamp is not None:  # a device tensor outside the range is clamped into it, on the device
        bad, good = clamp
        assert torch.equal(encode(pad, torch.tensor(bad, device=dev)), encode(pad, list(good)))
    return got


# ------------------------------------------------------------------------------------------------ mel front ends
def test_logmel_rows_are_the_rows_alone():
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec().to(dev)
    T, lens = 2400, [2400, 2399, 1600, 1599, 640, 513]
    assert codec.frame_lens(lens) == [16, 15, 11, 10, 5, 4]
    _check_rows(lambda w, l: codec.encode(w, lens=l) if l is not None else codec.encode(w), codec.frame_lens, lens, T,
                clamp=([0, T + 7] + lens[2:], [513, T] + lens[2:]))


def test_hifigan_mel_rows_are_the_rows_alone():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.codec import melspec_min_samples

    codec = vbx.HiFiGANMelCodec(n_fft=256, hop_size=64, win_size=256, num_mels=80, sampling_rate=22050, mean=-4.0, std=2.0).to(dev)
    lens = [1000, 999, 960, 640, 97]
    assert melspec_min_samples(256, 64) == 97
    _check_rows(lambda w, l: codec.encode(w, lens=l) if l is not None else codec.encode(w), codec.frame_lens, lens, 1000,
                clamp=([0, 1007] + lens[2:], [97, 1000] + lens[2:]))


# ------------------------------------------------------------------------------------------------ resample
@pytest.mark.parametrize("orig,new", [(16000, 24000), (44100, 24000)])
def test_resample_rows_are_the_rows_alone(orig, new):
    import voicebox_pytorch_amd as vbx

    L, lens = 3000, [3000, 1471, 1]
    fl = lambda l: vbx.resample_lens(l, orig, new)
    _check_rows(lambda w, l: vbx.resample(w, orig, new, lens=l) if l is not None else vbx.resample(w, orig, new), fl, lens, L,
                clamp=([3001, 1471, 0], [3000, 1471, 1]))


# ------------------------------------------------------------------------------------------------ SEANet
def _seanet(cls_name, cfg, seed=0):
    import voicebox_pytorch_amd as vbx

    kw = {k: cfg[k] for k in ("dimension", "n_filters", "n_residual_layers", "ratios", "lstm")}
    enc = getattr(vbx, cls_name)(**kw)
    enc.load_state_dict(S.random_state(cfg, seed))
    return enc.to(dev).eval()


@pytest.mark.parametrize("cls_name", ["SEANetEncoder", "CausalSEANetEncoder"])
@pytest.mark.parametrize("n_res", [1, 3])
def test_seanet_small_rows_are_the_rows_alone(cls_name, n_res):
    """hop 8; the short-input rule (1, 3, 7), `extra` on (7, 13, 1003) and off (8, 192), 16-position tile edges at the deepest layer"""
    enc = _seanet(cls_name, dict(S.SMALL, n_residual_layers=n_res))
    lens = list(C.ENC_T)
    _check_rows(lambda w, l: enc(w, lens=l) if l is not None else enc(w), enc.frame_lens, lens, max(lens), clamp=(
        [0] + lens[1:-1] + [max(lens) + 9], [1] + lens[1:]))


@pytest.mark.parametrize("cls_name", ["SEANetEncoder", "CausalSEANetEncoder"])
def test_seanet_24khz_widths_rows_are_the_rows_alone(cls_name):
    enc = _seanet(cls_name, S.config())
    lens = [24000, 5121]
    assert enc.frame_lens(lens) == [75, 17]
    _check_rows(lambda w, l: enc(w, lens=l) if l is not None else enc(w), enc.frame_lens, lens, 24000)


def _encodec(seed=0):
    import voicebox_pytorch_amd as vbx

    enc = _seanet("SEANetEncoder", S.SMALL, seed)
    g = torch.Generator().manual_seed(seed)
    rvq = vbx.ResidualVQ(dim=32, codebook_size=64, num_quantizers=4)
    rvq.load_state_dict({"codebooks": 0.5 ** torch.arange(4.0)[:, None, None] * torch.randn(4, 64, 32, generator=g)})
    voc = vbx.VocosDecoder(input_channels=32, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64)
    return vbx.EncodecVocoCodec(rvq=rvq, vocoder=voc, encoder=enc, downsample_factor=enc.hop_length).to(dev).eval()


def test_encodec_codec_rows_are_the_rows_alone():
    codec = _encodec()
    lens = [190, 131, 8, 5]
    _check_rows(lambda w, l: codec.encode(w, lens=l) if l is not None else codec.encode(w), codec.frame_lens, lens, 190)


# ------------------------------------------------------------------------------------------------ wrapper, train step, sampler
def _model(codec, seed=0):
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(seed)
    vb = vbx.VoiceBox(dim=64, depth=2, dim_head=64, heads=2, audio_enc_dec=codec, condition_on_text=False).to(dev)
    return vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb, resample_input=True)


def _draws(B, N, D, seed=7):
    g = torch.Generator().manual_seed(seed)
    return dict(x0=torch.randn(B, N, D, generator=g), times=torch.rand(B, generator=g), frac_lengths=0.7 + 0.3 * torch.rand(B, generator=g),
                rand=torch.rand(B, generator=g))


PLUMB_T, PLUMB_LENS = 2400, [2400, 1599, 640, 513]


def _loss_and_grads(wrapper, vb, draws, *args, **kw):
    from voicebox_pytorch_amd.masks import rng_override

    vb.zero_grad(set_to_none=True)
    with rng_override(**draws):
        loss = wrapper(*args, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in vb.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", ["list", "device"])
def test_wrapper_wave_lens_is_the_lens_path_on_latents(kind):
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec().to(dev)
    vb, wrapper = _model(codec)
    pad, _ = _waves(PLUMB_LENS, PLUMB_T)
    L = PLUMB_LENS if kind == "list" else torch.tensor(PLUMB_LENS, device=dev)
    F = codec.frame_lens(L)
    draws = _draws(len(PLUMB_LENS), 16, 100)
    la, ga = _loss_and_grads(wrapper, vb, draws, pad, wave_lens=L)
    lb, gb = _loss_and_grads(wrapper, vb, draws, codec.encode(pad, lens=L), lens=F)
    assert bool(torch.isfinite(la)) and torch.equal(la, lb), (float(la), float(lb))
    assert ga.keys() == gb.keys() and len(ga) > 10
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    # the padding is masked: the zero-padded batch without lengths trains on other numbers
    lc, _ = _loss_and_grads(wrapper, vb, draws, torch.nan_to_num(pad, nan=0.0))
    assert not torch.equal(la, lc)


def test_wrapper_wave_lens_resamples_from_16k():
    """resample_input=True: resample(lens=) and resample_lens in front of the codec"""
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec().to(dev)
    vb, wrapper = _model(codec)
    lens16 = [1600, 1066, 500, 342]  # -> 2400, 1599, 750, 513 samples at 24 kHz
    pad, _ = _waves(lens16, 1600)
    L24 = vbx.resample_lens(lens16, 16000, 24000)
    assert L24 == [2400, 1599, 750, 513]
    lat = codec.encode(vbx.resample(pad, 16000, 24000, lens=lens16), lens=L24)
    draws = _draws(4, 16, 100)
    la, ga = _loss_and_grads(wrapper, vb, draws, pad, wave_lens=lens16, input_sampling_rate=16000)
    lb, gb = _loss_and_grads(wrapper, vb, draws, lat, lens=codec.frame_lens(L24))
    assert bool(torch.isfinite(la)) and torch.equal(la, lb), (float(la), float(lb))
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]


def test_train_step_wave_lens_updates_like_the_lens_step():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override

    pad, _ = _waves(PLUMB_LENS, PLUMB_T)
    draws = _draws(len(PLUMB_LENS), 16, 100)
    out = []
    for use_waves in (True, False):
        codec = vbx.LogMelCodec().to(dev)
        vb, wrapper = _model(codec)
        ts = TrainStep(wrapper, lr=1e-3, max_grad_norm=0.5, length_bucket=64)
        with rng_override(**draws):
            if use_waves:
                loss = ts.step(pad, wave_lens=torch.tensor(PLUMB_LENS, device=dev))
            else:
                loss = ts.step(codec.encode(pad, lens=PLUMB_LENS), lens=codec.frame_lens(PLUMB_LENS))
        torch.cuda.synchronize()
        assert bool(ts._last_eng.io.key_lens)  # the lengths reached the runtime
        out.append((loss.detach().clone(), {k: v.detach().clone() for k, v in vb.state_dict().items()}))
    (la, sa), (lb, sb) = out
    assert bool(torch.isfinite(la)) and torch.equal(la, lb), (float(la), float(lb))
    assert all(torch.equal(sa[k], sb[k]) for k in sa), [k for k in sa if not torch.equal(sa[k], sb[k])]


def test_sample_wave_lens_is_sample_lens_on_latents():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    codec = vbx.LogMelCodec().to(dev)
    vb, wrapper = _model(codec)
    pad, _ = _waves(PLUMB_LENS, PLUMB_T)
    y0 = torch.randn(len(PLUMB_LENS), 16, 100, generator=torch.Generator().manual_seed(3))
    with rng_override(y0=y0):
        a = wrapper.sample(cond=pad, wave_lens=PLUMB_LENS, steps=2, decode_to_audio=False)
    with rng_override(y0=y0):
        b = wrapper.sample(cond=codec.encode(pad, lens=PLUMB_LENS), lens=codec.frame_lens(PLUMB_LENS), steps=2, decode_to_audio=False)
    with rng_override(y0=y0):
        c = wrapper.sample(cond=pad, wave_lens=torch.tensor(PLUMB_LENS, device=dev), steps=2, decode_to_audio=False)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c)
    assert wrapper.last_sample_lens.tolist() == codec.frame_lens(PLUMB_LENS)
    # pack=True and length_bucket work unchanged behind the encoded lengths
    for kw in (dict(pack=True), dict(length_bucket=64)):
        with rng_override(y0=y0):
            p = wrapper.sample(cond=pad, wave_lens=PLUMB_LENS, steps=2, decode_to_audio=False, **kw)
        with rng_override(y0=y0):
            q = wrapper.sample(cond=codec.encode(pad, lens=PLUMB_LENS), lens=codec.frame_lens(PLUMB_LENS), steps=2, decode_to_audio=False, **kw)
        assert bool(torch.isfinite(p).all()) and torch.equal(p, q), kw
