"""LogMelCodec.encode (csrc/mel.hip: framing, window, FFT in the LDS, mel filters, dB -- one kernel) against the fp64 restatement
tests/mel_ref.py.  Tolerance: what the reference's own arithmetic loses -- the same restatement in fp32 on the CPU, computed HERE on
the same input -- times 2 (a different summation order).  Parity with torchaudio itself is UNPINNED (tests/mel_ref.py)."""
import pytest
import torch

import mel_ref

pytestmark = pytest.mark.gpu
dev = "cuda"


def _check(a, factor=2.0, **kw):
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec(**kw).to(dev)
    got = codec.encode(a.to(dev)).double().cpu()
    log = kw.get("log", True)
    ref64 = mel_ref.log_mel(a, dtype=torch.float64, **kw)
    ref32 = mel_ref.log_mel(a, dtype=torch.float32, **kw).double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if log:
        err, cpu = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
        p64, p32, pg = 10 ** (ref64 / 10), 10 ** (ref32 / 10), 10 ** (got / 10)
    else:
        err = cpu = None
        p64, p32, pg = ref64, ref32, got
    rerr, rcpu = float(((pg - p64).abs() / p64).max()), float(((p32 - p64).abs() / p64).max())
    print(f"logmel {kw} T={a.shape[1]}: max |dB err| kernel {err} fp32-CPU {cpu}; max rel power err kernel {rerr:.3e} fp32-CPU {rcpu:.3e}; "
          f"range {float(ref64.min()):.1f} .. {float(ref64.max()):.1f}")
    if log:
        assert err <= factor * cpu, (err, cpu)
    assert rerr <= factor * rcpu, (rerr, rcpu)
    return got


def test_default_codec_vs_fp64():
    a = mel_ref.test_signal()
    got = _check(a)
    assert got.shape == (2, 151, 100)


@pytest.mark.parametrize("n_fft,win,hop", [(256, 160, 64), (512, 400, 128), (2048, 1200, 300)])
def test_other_fft_sizes(n_fft, win, hop):
    _check(mel_ref.test_signal(), n_fft=n_fft, win_length=win, hop_length=hop, n_mels=64)


def test_length_not_a_multiple_of_hop_and_power_output():
    a = mel_ref.test_signal()
    got = _check(a[:, :12345])
    assert got.shape == (2, 1 + 12345 // 160, 100)
    _check(a, log=False)


def test_short_wave_raises_as_reflect_padding_does():
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec().to(dev)
    with pytest.raises(RuntimeError):
        codec.encode(torch.zeros(1, 512, device=dev))
    with pytest.raises(RuntimeError):
        torch.stft(torch.zeros(1, 512), 1024, 160, 640, torch.hann_window(640), center=True, pad_mode="reflect", return_complex=True)
    assert codec.encode(torch.randn(1, 513, device=dev)).shape == (1, 4, 100)
    with pytest.raises(NotImplementedError):
        vbx.LogMelCodec(n_fft=1000)


def test_repeats_are_bit_identical_and_silence_is_minus_100_db():
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec().to(dev)
    a = mel_ref.test_signal().to(dev)
    assert torch.equal(codec.encode(a), codec.encode(a))
    s = codec.encode(torch.zeros(2, 4000, device=dev))
    assert float((s + 100.0).abs().max()) <= 100.0 * 2.0 ** -23, float((s + 100.0).abs().max())


def test_voicebox_with_logmel_codec_end_to_end():
    """VoiceBox(audio_enc_dec=LogMelCodec()): a training forward / backward from waves with gradients on proj_in, a sample to latents
    [B, 151, 100], and decode through a stand-in vocoder."""
    import voicebox_pytorch_amd as vbx

    class Vocoder(torch.nn.Module):  # stand-in: mel [B, n_mels, frames] -> wave [B, frames * hop]
        def forward(self, mel):
            return mel.mean(dim=1, keepdim=True).repeat(1, 160, 1).transpose(1, 2).reshape(mel.shape[0], -1)

    torch.manual_seed(0)
    codec = vbx.LogMelCodec(vocoder=Vocoder())
    vb = vbx.VoiceBox(dim=64, audio_enc_dec=codec, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False).to(dev)
    assert vb.proj_in.weight.shape == (64, 100) and vb.to_pred.weight.shape == (100, 64)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    wave = mel_ref.test_signal().to(dev)
    loss = wrapper(wave)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in vb.parameters() if p.grad is not None)
    assert float(vb.proj_in.weight.grad.abs().max()) > 0 and float(vb.proj_in.bias.grad.abs().max()) > 0
    s = wrapper.sample(cond=wave, steps=3, decode_to_audio=False)
    assert s.shape == (2, 151, 100) and torch.isfinite(s).all()
    w = wrapper.sample(cond=wave, steps=3)
    assert w.shape == (2, 151 * 160) and torch.isfinite(w).all()
    with pytest.raises(NotImplementedError):
        vbx.LogMelCodec().decode(s)
