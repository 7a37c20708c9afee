"""HiFiGANMelCodec.encode / mel_spectrogram (csrc/mel.hip, vbx_melspec: reflect pad, center=False framing, window, FFT in the LDS,
magnitude, Slaney filters, ln -- one kernel) against the fp64 restatement tests/hifigan_mel_ref.py, at the smallest shapes that reach
every edge (hifigan_mel_ref.CASES).  Tolerance, the rule of tests/test_mel_gpu.py: what the arithmetic itself loses -- the same
restatement in fp32 on the CPU, computed on the same input -- times 2 (a different summation order), on ln mel and on the relative
error of mel.  tests/test_hifigan_mel_cpu.py measures that this is under a tenth of what the smallest planted fault moves.  Parity
with HiFi-GAN / BigVGAN / librosa themselves is UNPINNED (tests/hifigan_mel_ref.py)."""
import math

import pytest
import torch

import hifigan_mel_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"


def _kw(cfg):
    return dict(n_fft=cfg["n_fft"], num_mels=cfg["num_mels"], sampling_rate=cfg["sr"], hop_size=cfg["hop"], win_size=cfg["win"],
                fmin=cfg["fmin"], fmax=cfg["fmax"])


def _ulp(x):
    """the spacing of fp32 at |x| (x fp64, normal range)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126))) - 23)


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_kernel_vs_fp64(name):
    import voicebox_pytorch_amd as vbx

    cfg, y, ref64, ref32 = R.case(name)
    ref32 = ref32.double()
    codec = vbx.HiFiGANMelCodec(**_kw(cfg))
    lat = codec.encode(y.to(dev))
    frames = R.frames_of(y.shape[1], cfg["n_fft"], cfg["hop"])
    assert lat.shape == (2, frames, cfg["num_mels"]) and lat.dtype == torch.float32 and lat.is_contiguous()
    if (cfg["n_fft"] - cfg["hop"]) % 2 == 0:
        assert frames == y.shape[1] // cfg["hop"]
    got = lat.transpose(1, 2).double().cpu()
    assert got.shape == ref64.shape and float(ref64.min()) > -11.0  # nothing near the clamp at ln 1e-5: nothing to mask out
    err, cpu = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    m64, m32, mg = ref64.exp(), ref32.exp(), got.exp()
    rerr, rcpu = float(((mg - m64).abs() / m64).max()), float(((m32 - m64).abs() / m64).max())
    print(f"melspec {name} T={y.shape[1]} frames={frames}: max |d ln mel| kernel {err:.3e} fp32-CPU {cpu:.3e}; max rel mel err kernel "
          f"{rerr:.3e} fp32-CPU {rcpu:.3e}; range {float(ref64.min()):.2f} .. {float(ref64.max()):.2f}")
    assert err <= 2.0 * cpu, (err, cpu)
    assert rerr <= 2.0 * rcpu, (rerr, rcpu)
    # channel-first (mel_spectrogram, what the generators take) is the same bits transposed
    cf = vbx.mel_spectrogram(y.to(dev), **_kw(cfg))
    assert cf.shape == (2, cfg["num_mels"], frames) and cf.is_contiguous() and torch.equal(cf, lat.transpose(1, 2))


def test_reruns_rows_and_input_forms_are_bit_equal():
    import voicebox_pytorch_amd as vbx

    codec = vbx.HiFiGANMelCodec()
    y = R.test_signal(1280 + 256 * 4 + 3, 22050, batch=3).to(dev)  # 9 frames: three workgroups per row, the last one partial
    a = codec.encode(y)
    assert a.shape == (3, 9, 80) and torch.equal(a, codec.encode(y))
    for b in range(3):
        assert torch.equal(codec.encode(y[b:b + 1]), a[b:b + 1]), b
    assert torch.equal(codec.encode(y[:, None]), a)  # [B, 1, T]
    assert torch.equal(codec.encode(y.double()), a) and torch.equal(codec.encode(y.t().contiguous().t()), a)
    cf = vbx.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000)
    assert torch.equal(cf, vbx.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000))
    assert torch.equal(cf[1:2], vbx.mel_spectrogram(y[1:2], 1024, 80, 22050, 256, 1024, 0, 8000))
    assert torch.equal(cf, a.transpose(1, 2))


def test_no_host_synchronisation():
    """encode and mel_spectrogram are one launch on tables already on the device: nothing waits for the GPU"""
    import voicebox_pytorch_amd as vbx

    codec = vbx.HiFiGANMelCodec(mean=-2.0, std=2.0)
    y = R.test_signal(5000, 22050).to(dev)
    warm = codec.encode(y)  # builds and caches the tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = codec.encode(y)
        b = vbx.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(a, warm) and b.shape == (2, 80, 19)


def test_normalisation_and_fit():
    """(x - mean) * (1 / std) in fp32 with 1 / std rounded once: three roundings, at most 2 ulp of the result from the exact
    (plain - mean) / std on the kernel's own plain output (fp32 mean and std)"""
    import voicebox_pytorch_amd as vbx

    y = R.test_signal(5000, 22050).to(dev)
    plain = vbx.HiFiGANMelCodec().encode(y)
    for mean, std in ((-1.75, 2.25), (0.3, 0.7), (-5.123, 1.0 / 3.0)):
        codec = vbx.HiFiGANMelCodec(mean=mean, std=std)
        got = codec.encode(y).double().cpu()
        m32, s32 = float(torch.tensor(mean, dtype=torch.float32)), float(torch.tensor(std, dtype=torch.float32))
        want = (plain.double().cpu() - m32) / s32
        worst = float(((got - want).abs() / _ulp(want)).max())
        print(f"normalised (mean {mean}, std {std}): worst {worst:.3f} ulp")
        assert worst <= 2.0, worst
    fit = vbx.HiFiGANMelCodec()
    mean, std = fit.fit_normalization([y, y[:1, :3000]])
    every = torch.cat((plain.flatten(), fit._encode(y[:1, :3000], None, None).flatten())).double()
    assert abs(mean - float(every.mean())) < 1e-9 and abs(std - float(every.std(unbiased=False))) < 1e-9
    assert (fit.mean, fit.std) == (mean, std)
    z = torch.cat((fit.encode(y).flatten(), fit.encode(y[:1, :3000]).flatten())).double()
    assert abs(float(z.mean())) < 1e-5 and abs(float(z.std(unbiased=False)) - 1.0) < 1e-5


def test_silence_is_ln_1e_minus_5():
    import voicebox_pytorch_amd as vbx

    s = vbx.HiFiGANMelCodec().encode(torch.zeros(2, 4000, device=dev)).double().cpu()
    want = torch.tensor(math.log(1e-5), dtype=torch.float64)
    assert s.shape == (2, 15, 80) and float((s - want).abs().max()) <= float(_ulp(want)), float((s - want).abs().max())


def test_short_waves_raise_where_f_pad_raises():
    import voicebox_pytorch_amd as vbx

    codec = vbx.HiFiGANMelCodec()
    for T in (1, 384):
        with pytest.raises(RuntimeError):
            torch.nn.functional.pad(torch.zeros(1, 1, T, device=dev), (384, 384), mode="reflect")
        with pytest.raises(RuntimeError):
            codec.encode(torch.zeros(1, T, device=dev))
        with pytest.raises(RuntimeError):
            vbx.mel_spectrogram(torch.zeros(1, T, device=dev), 1024, 80, 22050, 256, 1024, 0, 8000)
    assert codec.encode(torch.randn(1, 385, device=dev)).shape == (1, 1, 80)
    with pytest.raises(RuntimeError):
        vbx.mel_spectrogram(torch.zeros(1, 255, device=dev), 256, 20, 22050, 256, 256, 0, None)
    assert vbx.mel_spectrogram(torch.zeros(1, 256, device=dev), 256, 20, 22050, 256, 256, 0, None).shape == (1, 20, 1)
    with pytest.raises(vbx._lib.VbxError):
        codec.encode(torch.zeros(1, 4000))


SMALL_GEN = dict(n_mels=80, upsample_initial_channel=128, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), resblock="1",
                 resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3),))
VB = dict(dim=64, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False)


def test_voicebox_with_hifigan_mel_codec_end_to_end():
    """wave -> the vocoder's mel -> VoiceBox training and sample() -> the same mel -> HiFiGANGenerator -> wave, random narrow weights"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep

    torch.manual_seed(0)
    gen = vbx.HiFiGANGenerator(**SMALL_GEN)
    codec = vbx.HiFiGANMelCodec(vocoder=gen, mean=-2.0, std=2.0)
    assert gen.hop_length == codec.downsample_factor == 256
    vb = vbx.VoiceBox(audio_enc_dec=codec, **VB).to(dev)
    assert vb.proj_in.weight.shape == (64, 80) and vb.to_pred.weight.shape == (80, 64)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, resample_input=True)
    T = 5000
    wave = R.test_signal(T, 22050).to(dev)
    loss = wrapper(wave)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in vb.parameters() if p.grad is not None)
    assert float(vb.proj_in.weight.grad.abs().max()) > 0 and float(vb.proj_in.bias.grad.abs().max()) > 0
    s = wrapper.sample(cond=wave, steps=3, decode_to_audio=False)
    assert s.shape == (2, T // 256, 80) and torch.isfinite(s).all()
    w = wrapper.sample(cond=wave, steps=3)
    assert w.shape == (2, (T // 256) * 256) and torch.isfinite(w).all()
    # decode is the generator on the de-normalised, transposed latents
    assert torch.equal(codec.decode(s), gen(s.transpose(1, 2) * 2.0 - 2.0))
    # one optimizer step from 16 kHz waves into the 22.05 kHz codec
    wave16 = R.test_signal(4000, 16000).to(dev)
    lat, _ = wrapper.encode_raw_audio(wave16, None, input_sampling_rate=16000)
    assert lat.shape == (2, -(-22050 * 4000 // 16000) // 256, 80)
    before = vb.proj_in.weight.detach().clone()
    l1 = TrainStep(wrapper, lr=1e-3, max_grad_norm=0.5).step(wave16, input_sampling_rate=16000)
    assert torch.isfinite(l1) and not torch.equal(vb.proj_in.weight.detach(), before)
    # the mismatch refusals of decode, with the real generators
    with pytest.raises(NotImplementedError):
        vbx.HiFiGANMelCodec().decode(s)
    with pytest.raises(ValueError, match="input_log"):
        vbx.HiFiGANMelCodec(vocoder=vbx.HiFiGANGenerator(**SMALL_GEN, input_log=True)).decode(s)
    with pytest.raises(ValueError, match="mel bins"):
        vbx.HiFiGANMelCodec(num_mels=100, vocoder=gen).decode(torch.zeros(2, 19, 100, device=dev))
    with pytest.raises(ValueError, match="hop_size"):
        vbx.HiFiGANMelCodec(hop_size=128, vocoder=gen).decode(s)


def test_from_checkpoint_pairs_generator_and_codec(tmp_path):
    """a HiFi-GAN file and a BigVGAN file (synthetic, random weights) with their config.json: the right generator class, the config's
    front end, and a wave of frames * hop samples out of decode(encode(wave))"""
    import json

    import voicebox_pytorch_amd as vbx

    torch.manual_seed(1)
    front = dict(num_mels=80, n_fft=1024, hop_size=256, win_size=1024, sampling_rate=22050, fmin=0, fmax=None, fmax_for_loss=None)
    gen_cfg = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=128,
                   resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3]])
    wave = R.test_signal(2000, 22050).to(dev)
    for extra, cls, make in ((dict(), vbx.HiFiGANGenerator, lambda: vbx.HiFiGANGenerator(**SMALL_GEN)),
                             (dict(activation="snakebeta", snake_logscale=True), vbx.BigVGANGenerator,
                              lambda: vbx.BigVGANGenerator(**SMALL_GEN))):
        cfg = dict(front, **gen_cfg, **extra)
        gpath, cpath = tmp_path / f"g_{cls.__name__}", tmp_path / f"config_{cls.__name__}.json"
        torch.save({"generator": make().state_dict()}, gpath)
        cpath.write_text(json.dumps(cfg))
        codec = vbx.HiFiGANMelCodec.from_checkpoint(gpath, cpath)
        assert type(codec.vocoder) is cls and codec.fmax == 11025.0 and codec.num_mels == 80 and not codec.training
        out = codec.decode(codec.encode(wave))
        assert out.shape == (2, (2000 // 256) * 256) and torch.isfinite(out).all()
