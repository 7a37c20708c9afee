"""voicebox_pytorch_amd.resample on the device (csrc/resample.hip) against the fp64 restatement tests/resample_ref.py, which uses
the same fp32-rounded filter bank.  The tolerance is DERIVED, not tuned: per output sample

    |got - ref64| <= (K + 1) * 2^-24 * sum_k |h[p][k] * x|

the forward-error bound of ANY fp32 summation order of K products (K roundings of the running sum and one of each product, first
order), with the right-hand side computed in fp64; the fp32 conv1d of the same restatement on the CPU is printed beside it.  Then the
edges, and the wiring of ConditionalFlowMatcherWrapper(resample_input=True) through forward, TrainStep and VoiceBoxTrainer.  Parity
with torchaudio itself is UNPINNED (tests/resample_ref.py)."""
import pytest
import torch

import resample_ref as R
from toy_codec import ToyCodec

pytestmark = pytest.mark.gpu
dev = "cuda"

PAIRS = [(16000, 24000), (44100, 24000), (48000, 24000), (22050, 24000), (8000, 24000), (24000, 16000), (48000, 11025), (11025, 48000)]
METHODS = ["sinc_interp_hann", "sinc_interp_kaiser"]
KAISER_BEST = dict(lowpass_filter_width=64, rolloff=0.9475937167399596, resampling_method="sinc_interp_kaiser", beta=14.769656459379492)
KW = dict(dim=64, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False, time_hidden_dim=64, ff_mult=2)


def _check(x, orig, new, what, fp32_cpu=True, **kw):
    """x fp32 [..., L] on the CPU -> the kernel's result (CPU tensor), checked against the bound above"""
    import voicebox_pytorch_amd as vbx

    got = vbx.resample(x.to(dev), orig, new, **kw)
    assert got.dtype == torch.float32 and got.device.type == "cuda"
    got = got.cpu()
    ref, s = R.resample(x, orig, new, return_bound=True, **kw)
    K = R.bank(orig, new, **kw)[0].shape[1]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = (K + 1) * 2.0 ** -24 * s
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    line = f"resample {what} {orig}->{new} {kw.get('resampling_method', 'sinc_interp_hann')} lpw {kw.get('lowpass_filter_width', 6)} " \
           f"shape {tuple(x.shape)} K {K}: max |err| {float(err.max()):.3e}, max |err| / bound {ratio:.4f}, min bound {float(bound.min()):.3e}"
    if fp32_cpu:
        e32 = (R.resample(x, orig, new, dtype=torch.float32, **kw).double() - ref).abs()
        line += f", fp32-CPU conv1d / bound {float((e32[live] / bound[live]).max()):.4f}"
    print(line)
    assert bool((err <= bound).all()), (what, orig, new, ratio)
    return got


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("orig,new", PAIRS)
def test_kernel_vs_fp64_restatement(orig, new, method):
    """noise + tone + chirp, 2 rows, one second at the source rate: the bound is never zero on it"""
    x = R.test_signal(batch=2, seconds=1.0, sampling_rate=orig)
    got = _check(x, orig, new, "parity", resampling_method=method)
    ro, rn = R.reduced(orig, new)
    assert got.shape == (2, -(-rn * orig // ro))


@pytest.mark.parametrize("orig,new", [(16000, 24000), (48000, 11025), (11025, 48000)])
def test_edge_lengths(orig, new):
    ro, rn = R.reduced(orig, new)
    K = R.bank(orig, new)[0].shape[1]
    for L in (1, K - 1, 7 * ro, 12345):
        x = R.test_signal(batch=2, seconds=L / orig + 1e-6, sampling_rate=orig, seed=L)[:, :L]
        assert x.shape == (2, L)
        _check(x, orig, new, f"L={L}")


def test_shapes_dtypes_and_views():
    import voicebox_pytorch_amd as vbx

    x = R.test_signal(batch=2, seconds=0.25, sampling_rate=16000)
    T = x.shape[1]
    y2 = vbx.resample(x.to(dev), 16000, 24000)
    y1 = vbx.resample(x[0].to(dev), 16000, 24000)
    y3 = vbx.resample(x[:, None].to(dev), 16000, 24000)
    assert y1.shape == (T * 3 // 2,) and y2.shape == (2, T * 3 // 2) and y3.shape == (2, 1, T * 3 // 2)
    assert torch.equal(y1, y2[0]) and torch.equal(y3[:, 0], y2)
    assert torch.equal(vbx.resample(x.to(dev), 16000, 24000), y2)  # two calls: the same bits
    assert torch.equal(vbx.Resample(16000, 24000)(x.to(dev)), y2)
    # a non-contiguous view gives what its contiguous copy gives
    wide = R.test_signal(batch=2, seconds=0.5, sampling_rate=16000).to(dev)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(vbx.resample(view, 16000, 24000), vbx.resample(view.contiguous(), 16000, 24000))
    # the rates are reduced by their gcd: 32000 -> 48000 is 16000 -> 24000 on the same samples
    assert torch.equal(vbx.resample(x.to(dev), 32000, 48000), y2)
    # zeros in, exact zeros out
    z = vbx.resample(torch.zeros(3, 5000, device=dev), 44100, 24000)
    assert z.shape == (3, 2722) and not z.any()
    # compute is fp32: other float dtypes are converted in and out
    y64 = vbx.resample(x.double().to(dev), 16000, 24000)
    assert y64.dtype == torch.float64 and torch.equal(y64, y2.double())
    y16 = vbx.resample(x.half().to(dev), 16000, 24000)
    assert y16.dtype == torch.float16 and torch.equal(y16, vbx.resample(x.half().float().to(dev), 16000, 24000).half())
    xd = x.to(dev)
    assert vbx.resample(xd, 24000, 24000) is xd  # equal rates: the input itself


@pytest.mark.parametrize("orig,new", [(16000, 24000), (44100, 24000), (48000, 11025)])
def test_wide_filters(orig, new):
    """lowpass_filter_width 16 and 64 (Hann), and torchaudio's documented "kaiser_best" settings"""
    x = R.test_signal(batch=2, seconds=0.5, sampling_rate=orig)
    for lpw in (16, 64):
        _check(x, orig, new, "wide", lowpass_filter_width=lpw)
    _check(x, orig, new, "kaiser_best", **KAISER_BEST)


def test_large_batch_of_long_rows():
    """8 x 163 840 samples, 16 k -> 24 k, under the same bound"""
    x = R.test_signal(batch=8, seconds=163840 / 16000, sampling_rate=16000)
    assert x.shape == (8, 163840)
    got = _check(x, 16000, 24000, "long", fp32_cpu=False)
    assert got.shape == (8, 245760)


# ------------------------------------------------------------------------------------ wiring
def _wrapper(codec, state=None, **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(audio_enc_dec=codec, **KW)
    if state is not None:
        vb.load_state_dict(state)
    return vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev), **kw)


def _draws(shape, seed=5):
    g = torch.Generator().manual_seed(seed)
    return dict(x0=torch.randn(shape, generator=g), times=torch.rand(shape[0], generator=g), frac_lengths=torch.tensor([0.8, 0.9]),
                rand=torch.rand(shape[0], generator=g))


def test_wrapper_resamples_input_and_cond():
    """resample_input=True: wrapper(wave16k, input_sampling_rate=16000) is wrapper(resample(wave16k)) bit for bit, for x1 and for a raw
    cond; off (the default), the same call raises as before."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    torch.manual_seed(7)
    on = _wrapper(ToyCodec(100), resample_input=True)
    off = _wrapper(ToyCodec(100), state=on.voicebox.state_dict())
    wave16 = R.test_signal(batch=2, seconds=428 / 16000 + 1e-6, sampling_rate=16000)[:, :428].to(dev)
    wave24 = vbx.resample(wave16, 16000, 24000)
    assert wave24.shape == (2, 642)
    draws = _draws((2, 40, 100))
    with rng_override(**draws):
        a = on(wave16, input_sampling_rate=16000)
        b = on(wave24)
        c = off(wave24, input_sampling_rate=24000)
        with pytest.raises(NotImplementedError, match="resample_input=True"):
            off(wave16, input_sampling_rate=16000)
    assert torch.isfinite(a) and torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), c.detach())
    lat = on.voicebox.audio_enc_dec.encode(wave24)
    with rng_override(**draws):
        a = on(lat, cond=wave16, input_sampling_rate=16000)
        b = on(lat, cond=wave24)
        d = on(lat, cond=wave24[:, None], input_sampling_rate=24000)
    assert torch.isfinite(a) and torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), d.detach())
    lat2, cond2 = on.encode_raw_audio(wave16, wave16, input_sampling_rate=16000)
    assert torch.equal(lat2, lat) and torch.equal(cond2, lat) and not lat2.requires_grad


def test_train_step_from_16k_waves():
    """TrainStep.step(wave16k, input_sampling_rate=16000) against the step from the resampled waves: the same loss and the same
    updated parameters, bit for bit"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override

    torch.manual_seed(8)
    w1 = _wrapper(ToyCodec(100), resample_input=True)
    start = {k: v.detach().cpu().clone() for k, v in w1.voicebox.state_dict().items()}
    w2 = _wrapper(ToyCodec(100), state=start, resample_input=True)
    wave16 = R.test_signal(batch=2, seconds=428 / 16000 + 1e-6, sampling_rate=16000, seed=3)[:, :428].to(dev)
    draws = _draws((2, 40, 100), seed=6)
    with rng_override(**draws):
        l1 = TrainStep(w1, lr=1e-3, max_grad_norm=0.5).step(wave16, input_sampling_rate=16000)
        l2 = TrainStep(w2, lr=1e-3, max_grad_norm=0.5).step(vbx.resample(wave16, 16000, 24000))
    assert torch.isfinite(l1) and torch.equal(l1.detach(), l2.detach())
    sd1, sd2 = w1.voicebox.state_dict(), w2.voicebox.state_dict()
    moved = 0
    for k in ("proj_in.weight", "proj_in.bias", "to_pred.weight", "to_embed.weight", "transformer.layers.0.3.to_qkv.weight"):
        assert torch.equal(sd1[k], sd2[k]), k
        moved += int(not torch.equal(sd1[k].cpu(), start[k]))
    assert moved == 5
    off = _wrapper(ToyCodec(100), state=start)
    with pytest.raises(NotImplementedError, match="resampl"):
        TrainStep(off, lr=1e-3).step(wave16, input_sampling_rate=16000)


def test_logmel_codec_latent_frames_from_16k():
    """LogMelCodec is a 24 kHz codec: T samples at 16 kHz become ceil(3 T / 2) samples and 1 + ceil(3 T / 2) // 160 frames"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    w = _wrapper(vbx.LogMelCodec(), resample_input=True)
    for T in (16000, 4001):
        wave16 = R.test_signal(batch=2, seconds=T / 16000 + 1e-6, sampling_rate=16000)[:, :T].to(dev)
        lat, _ = w.encode_raw_audio(wave16, None, input_sampling_rate=16000)
        n24 = -(-3 * T // 2)
        assert lat.shape == (2, 1 + n24 // 160, 100) and torch.isfinite(lat).all()
        assert torch.equal(lat, w.voicebox.audio_enc_dec.encode(vbx.resample(wave16, 16000, 24000)))
    with rng_override(**_draws(tuple(lat.shape))):
        loss = w(wave16, input_sampling_rate=16000)
    assert torch.isfinite(loss)


def test_trainer_on_a_16k_wave_dataset(tmp_path):
    import voicebox_pytorch_amd as vbx

    class Waves(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return torch.randn(428, generator=torch.Generator().manual_seed(i))

    torch.manual_seed(0)
    tr = vbx.VoiceBoxTrainer(_wrapper(ToyCodec(100), resample_input=True), batch_size=2, dataset=Waves(), num_train_steps=10,
                             num_warmup_steps=2, lr=1e-3, valid_frac=0.25, results_folder=str(tmp_path / "r"), log_every=100,
                             save_results_every=1, save_model_every=100, force_clear_prev_results=True, input_sampling_rate=16000)
    for _ in range(2):
        logs = tr.train_step()
        assert logs["loss"] == logs["loss"] and abs(logs["loss"]) < float("inf")
        assert logs["valid_loss"] == logs["valid_loss"] and abs(logs["valid_loss"]) < float("inf")
    plain = vbx.VoiceBoxTrainer(_wrapper(ToyCodec(100)), batch_size=2, dataset=Waves(), num_train_steps=10, num_warmup_steps=2, lr=1e-3,
                                valid_frac=0.25, results_folder=str(tmp_path / "p"), log_every=100, save_results_every=100,
                                save_model_every=100, force_clear_prev_results=True, input_sampling_rate=16000)
    with pytest.raises(NotImplementedError, match="resampl"):
        plain.train_step()
