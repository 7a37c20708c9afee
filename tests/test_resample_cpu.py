"""CPU (-m "not gpu") side of voicebox_pytorch_amd.resample: the fp64 restatement (tests/resample_ref.py) against a per-sample
evaluation without bank or convolution and against the analytic resampling of a sine; the product's fp32 filter bank and its
per-phase non-zero runs against the restatement's; host behaviour (lengths, gcd reduction, argument checks, the bank cap, no state,
the resample_input switch of the wrapper on paths that launch nothing).  PARITY UNPINNED with torchaudio: see resample_ref.py."""
import math

import pytest
import torch

import resample_ref as R
from toy_codec import ToyCodec

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
KW = dict(dim=64, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False, time_hidden_dim=64, ff_mult=2)


@pytest.mark.parametrize("method", ["sinc_interp_hann", "sinc_interp_kaiser"])
@pytest.mark.parametrize("orig,new", [(16000, 24000), (24000, 16000)])
def test_restatement_against_direct_evaluation(orig, new, method):
    """<= 1e-12 (fp64 summation order is all that may differ) on 300 samples of the test signal"""
    x = R.test_signal(1, 300 / orig + 1e-9, orig)[0, :300]
    got = R.resample(x, orig, new, resampling_method=method, round_bank=False)
    want = R.resample_direct(x, orig, new, resampling_method=method)
    err = float((got - want).abs().max())
    print(f"restatement vs direct {orig}->{new} {method}: {err:.3e}")
    assert got.shape == want.shape == (300 * new // orig,) and err <= 1e-12


@pytest.mark.parametrize("method,orig,bound", [("sinc_interp_hann", o, 1e-3) for o in (16000, 44100, 48000, 22050, 8000)]
                         + [("sinc_interp_kaiser", 16000, 1e-6), ("sinc_interp_kaiser", 44100, 1e-6)])
def test_sine_reproduction(method, orig, bound):
    """A unit 440 Hz sine resampled to 24 kHz against the same sine sampled at 24 kHz, 200 samples skipped at each end.  The bounds
    are properties of the published filter (pass-band ripple of a width-6 Hann-windowed sinc at 0.99 roll-off: a few 1e-4; the Kaiser
    window at beta 14.77: below 1e-7), not of any code under test."""
    new = 24000
    x = torch.sin(2 * math.pi * 440 * torch.arange(orig, dtype=torch.float64) / orig)
    y = R.resample(x, orig, new, resampling_method=method, round_bank=False)
    want = torch.sin(2 * math.pi * 440 * torch.arange(new, dtype=torch.float64) / new)
    err = float((y - want)[200:-200].abs().max())
    print(f"sine {orig}->{new} {method}: {err:.3e}")
    assert y.shape == (new,) and err <= bound


@pytest.mark.parametrize("method", ["sinc_interp_hann", "sinc_interp_kaiser"])
def test_product_bank_against_restatement(method):
    """every ordered pair of the common rates: the product's bank within one fp32 rounding of the restatement's, and the per-phase
    runs cover exactly the taps that are not 0.0 in fp32.  Every dense bank is far below the 16 MiB cap: the largest is 11025 -> 32000
    (1280 phases x 455 taps, 2.3 MB), 11025 -> 48000 has 640 x 161, the deepest filter is 48000 -> 11025 with 694 taps."""
    from voicebox_pytorch_amd.codec import resample_bank

    worst, dense_max = 0.0, 0
    for orig in RATES:
        for new in RATES:
            if orig == new:
                continue
            h, width, start, length = resample_bank(orig, new, resampling_method=method)
            ref, rwidth = R.bank(orig, new, resampling_method=method)
            ro, rn = R.reduced(orig, new)
            assert h.dtype == torch.float32 and tuple(h.shape) == tuple(ref.shape) == (rn, 2 * width + ro) and width == rwidth
            err, scale = float((h.double() - ref.float().double()).abs().max()), float(ref.abs().max())
            worst = max(worst, err / scale)
            assert err <= 2.0 ** -24 * scale, (orig, new, err, scale)
            k = torch.arange(h.shape[1])[None, :]
            run = (k >= start[:, None]) & (k < (start + length)[:, None])
            assert torch.equal(run, h != 0), (orig, new)
            assert int(length.min()) >= 1 and int((start + length).max()) <= h.shape[1]
            if method == "sinc_interp_kaiser":
                assert int(length.min()) == h.shape[1]
            dense_max = max(dense_max, h.numel() * 4)
    print(f"bank {method}: worst |diff| / max|h| = {worst:.3e}, largest dense bank {dense_max} bytes")
    assert dense_max == 1280 * 455 * 4
    h, _, start, length = resample_bank(11025, 48000)
    assert tuple(h.shape) == (640, 161)
    assert resample_bank(48000, 11025)[0].shape[1] == 694
    if method == "sinc_interp_hann":  # the recorded fill of the deep Hann banks
        for (o, n), lo, hi in (((22050, 24000), 0.07, 0.08), ((44100, 24000), 0.125, 0.135), ((48000, 11025), 0.07, 0.08)):
            h = resample_bank(o, n)[0]
            assert lo < float((h != 0).float().mean()) < hi, (o, n, float((h != 0).float().mean()))


def test_device_tables_hold_the_runs():
    """the compacted run-major bank handed to the kernel, rebuilt dense, is the bank"""
    from voicebox_pytorch_amd import codec

    for orig, new, method in ((147, 80, "sinc_interp_hann"), (640, 147, "sinc_interp_hann"), (2, 3, "sinc_interp_kaiser")):
        taps, start, length, width, K, run_max = codec._resample_tables(orig, new, 6, 0.99, method, None, "cpu")
        h = codec.resample_bank(orig, new, resampling_method=method)[0]
        assert tuple(taps.shape) == (run_max, new) and K == h.shape[1] == 2 * width + orig and run_max == int(length.max())
        dense = torch.zeros_like(h)
        for p in range(new):
            s, n = int(start[p]), int(length[p])
            dense[p, s:s + n] = taps[:n, p]
            assert not taps[n:, p].any()
        assert torch.equal(dense, h)
    n0 = len(codec._resample_tables_cache)
    assert codec._resample_tables(2, 3, 6, 0.99, "sinc_interp_kaiser", None, "cpu")[0] is taps  # cached
    assert len(codec._resample_tables_cache) == n0 <= 8 and isinstance(codec._resample_tables_cache, dict)


def test_host_behaviour():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.codec import resample_bank

    x = torch.randn(2, 100)
    assert vbx.resample(x, 16000, 16000) is x
    assert vbx.resample(x, 48000, 48000.0) is x
    assert vbx.Resample(24000, 24000)(x) is x
    # gcd reduction: the same bank for 32000 -> 48000 as for 2 -> 3
    a, b = resample_bank(32000, 48000), resample_bank(2, 3)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] == 7 and tuple(a[0].shape) == (3, 16)
    # output length ceil(new L / orig) on the reduced pair (the restatement keeps the same number)
    for orig, new, L in ((16000, 24000, 1), (16000, 24000, 301), (48000, 11025, 1000), (11025, 48000, 77), (44100, 24000, 441)):
        ro, rn = R.reduced(orig, new)
        assert R.resample(torch.zeros(L), orig, new).shape == (-(-rn * L // ro),)
    for bad in (dict(orig_freq=16000.5, new_freq=24000), dict(orig_freq=16000, new_freq=0.5)):
        with pytest.raises(Exception, match="integ"):
            vbx.resample(x, **bad)
    for bad in (dict(orig_freq=0, new_freq=24000), dict(orig_freq=16000, new_freq=-1), dict(orig_freq=-16000, new_freq=-16000)):
        with pytest.raises(ValueError):
            vbx.resample(x, **bad)
    with pytest.raises(ValueError, match="lowpass_filter_width"):
        vbx.resample(x, 16000, 24000, lowpass_filter_width=0)
    with pytest.raises(ValueError, match="resampling_method"):
        vbx.resample(x, 16000, 24000, resampling_method="sinc_interp_boxcar")
    with pytest.raises(ValueError):
        vbx.Resample(16000, 24000, resampling_method="nearest")
    with pytest.raises(NotImplementedError, match="MiB"):  # near-coprime: 24000 phases x 48025 taps
        resample_bank(24001, 24000)
    with pytest.raises(TypeError):
        vbx.resample(torch.zeros(2, 100, dtype=torch.int16), 16000, 24000)
    with pytest.raises(_lib.VbxError, match="MI355X"):  # no CPU fallback, as griffin_lim
        vbx.resample(x, 16000, 24000)
    m = vbx.Resample(16000, 24000)
    assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    assert _lib.lib().vbx_resample_max_taps() == 16384
    # the entry point checks its arguments on the host, before any launch
    with pytest.raises(_lib.VbxError, match="vbx_resample"):
        _lib.call("vbx_resample", None, None, None, None, None, 1, 100, 150, 2, 3, 7, 16, 13, None)


def test_resample_input_switch_without_a_launch():
    """resample_input=True at equal rates, with no rate, and with latents passes through untouched (a CPU box: a launch would
    raise); off, a differing rate raises as before and names the switch."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    codec = ToyCodec(100)
    on = vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(audio_enc_dec=codec, **KW), resample_input=True)
    off = vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(audio_enc_dec=ToyCodec(100), **KW))
    assert on.resample_input is True and off.resample_input is False
    assert set(on.state_dict()) == set(off.state_dict())
    wave = torch.randn(2, 640)
    want = codec.encode(wave)
    for rate in (None, 24000):
        lat, cond = on.encode_raw_audio(wave, wave[:, None], input_sampling_rate=rate)
        assert torch.equal(lat, want) and torch.equal(cond, want)
    x, c = on.encode_raw_audio(want, None, input_sampling_rate=16000)  # latents: nothing to resample
    assert x is want and c is None
    with pytest.raises(NotImplementedError, match="resampl.*resample_input=True"):
        off.encode_raw_audio(wave, None, input_sampling_rate=16000)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.VbxError, match="MI355X"):
            on.encode_raw_audio(wave, None, input_sampling_rate=16000)
    # the trainer hands its rate to the step
    from voicebox_pytorch_amd.trainer import VoiceBoxTrainer

    t = VoiceBoxTrainer.__new__(VoiceBoxTrainer)
    torch.nn.Module.__init__(t)
    t.cfm_wrapper, t.input_sampling_rate = on, 16000
    x, kw = t._model_kwargs((wave,))
    assert x is wave and kw == dict(input_sampling_rate=16000)
    t.input_sampling_rate = None
    assert t._model_kwargs((wave,))[1] == {}
