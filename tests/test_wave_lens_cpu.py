"""Host side of ragged waves (voicebox_pytorch_amd/wave_lens.py, data.py): the frame_lens / resample_lens arithmetic against the
shapes encode gives, every refusal and validation message on a CPU wrapper (before anything could be launched), the trainer's collate
output reaching the step keywords under mask_wave_padding, AudioDataset over a tmp_path tree written with the stdlib, and the TEETH of
tests/test_wave_lens_gpu.py: how far the fp64 restatements move a row's last live frames when the row is zero-padded to the batch
length first, beside the restatements' own agreement with the device kernels.  Lines that start with PARITY are measured figures."""
import struct
import wave as wavelib

import pytest
import torch

import mel_ref
import seanet_causal_ref as C
import seanet_ref as S
from toy_codec import ToyCodec


# ------------------------------------------------------------------------------------------------ length arithmetic
def test_logmel_frame_lens_is_the_frame_count_of_encode():
    """1 + l // hop against the restatement's output shape (torch.stft, center=True) for every length of a range"""
    import voicebox_pytorch_amd as vbx

    for kw in (dict(), dict(n_fft=256, win_length=160, hop_length=64, n_mels=64)):
        codec = vbx.LogMelCodec(**kw)
        lens = list(range(codec.n_fft // 2 + 1, codec.n_fft // 2 + 1 + 3 * codec.hop_length + 2))
        F = codec.frame_lens(lens)
        for l, f in zip(lens, F):
            got = mel_ref.log_mel(torch.zeros(1, l), n_fft=codec.n_fft, win_length=codec.win_length, hop_length=codec.hop_length,
                                  n_mels=codec.n_mels).shape[1]
            assert f == got == 1 + l // codec.hop_length, (l, f, got)
        assert codec.frame_lens(torch.tensor(lens)).tolist() == F and codec.frame_lens(torch.tensor(lens)).dtype == torch.int64
        assert codec.frame_lens(torch.tensor(lens, dtype=torch.int32)).dtype == torch.int32


def test_hifigan_frame_lens_is_the_frame_count_of_encode():
    """melspec_frames against the frames an explicit center=False framing over the reflect pad holds"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.codec import melspec_min_samples, melspec_pad

    for n_fft, hop in ((256, 64), (1024, 256), (512, 100)):
        codec = vbx.HiFiGANMelCodec(n_fft=n_fft, hop_size=hop, win_size=n_fft, num_mels=80)
        lo, pad = melspec_min_samples(n_fft, hop), melspec_pad(n_fft, hop)
        lens = list(range(lo, lo + 3 * hop + 2))
        for l, f in zip(lens, codec.frame_lens(lens)):
            padded = torch.nn.functional.pad(torch.zeros(1, 1, l), (pad, pad), mode="reflect")[0]
            assert f == padded.unfold(-1, n_fft, hop).shape[1] >= 1, (n_fft, hop, l, f)
        assert codec.frame_lens(torch.tensor(lens)).tolist() == codec.frame_lens(lens)


@pytest.mark.parametrize("ratios", [(8, 5, 4, 2), (4, 2)])
@pytest.mark.parametrize("causal", [False, True])
def test_seanet_frame_lens_is_the_ceil_chain(ratios, causal):
    """against frames() for every length of a range, and against the restatement's output shape on a few"""
    import voicebox_pytorch_amd as vbx

    enc = (vbx.CausalSEANetEncoder if causal else vbx.SEANetEncoder)(n_filters=16, ratios=ratios, dimension=32)
    lens = list(range(1, 2 * enc.hop_length + 3))
    assert enc.frame_lens(lens) == [enc.frames(l) for l in lens]
    assert enc.frame_lens(torch.tensor(lens)).tolist() == enc.frame_lens(lens)
    if ratios == (4, 2):
        cfg = dict(S.SMALL)
        sd = S.random_state(cfg, 0)
        for l in (1, 7, 8, 9, 19):
            ref = (C if causal else S).encode(sd, cfg, torch.zeros(1, l))
            assert ref.shape[1] == enc.frame_lens([l])[0], (l, ref.shape)
    rvq = vbx.ResidualVQ(dim=32, codebook_size=64, num_quantizers=2)
    codec = vbx.EncodecVocoCodec(rvq=rvq, vocoder=None, encoder=enc)
    assert codec.frame_lens(lens) == enc.frame_lens(lens)


def test_resample_lens_is_the_ceiling():
    import voicebox_pytorch_amd as vbx

    lens = list(range(1, 700)) + [16000, 44100, 48000, 163840, 2 ** 31 - 1]
    for orig in (16000, 44100, 48000):
        got = vbx.resample_lens(lens, orig, 24000)
        assert got == [-(-24000 * l // orig) for l in lens]
        t = vbx.resample_lens(torch.tensor(lens), orig, 24000)
        assert t.dtype == torch.int64 and t.tolist() == got
    assert vbx.resample_lens(lens, 24000, 24000) == lens
    with pytest.raises(ValueError, match="integral"):
        vbx.resample_lens([5], 22050.5, 24000)
    with pytest.raises(ValueError, match="must hold ints"):
        vbx.resample_lens([5.0], 16000, 24000)


# ------------------------------------------------------------------------------------------------ validation of the front ends
def test_front_ends_validate_host_lengths_and_name_the_row():
    """a list or a CPU tensor is checked on the host, before the device is asked for: ValueError naming the row, the codec's own
    minimum as the lower end"""
    import voicebox_pytorch_amd as vbx

    mel = vbx.LogMelCodec()
    w = torch.zeros(3, 2400)
    with pytest.raises(ValueError, match=r"LogMelCodec\.encode: lens\[1\] = 512 is outside 513 \.\. T = 2400"):
        mel.encode(w, lens=[2400, 512, 600])
    with pytest.raises(ValueError, match=r"lens\[2\] = 2401 is outside 513 \.\. T = 2400"):
        mel.encode(w, lens=torch.tensor([2400, 513, 2401]))
    with pytest.raises(ValueError, match="one entry per batch row"):
        mel.encode(w, lens=[2400, 600])
    with pytest.raises(ValueError, match="int tensor"):
        mel.encode(w, lens=torch.tensor([2400., 600., 600.]))
    with pytest.raises(vbx._lib.VbxError, match="runs only on an MI355X"):  # valid lengths: the next check is the device
        mel.encode(w, lens=[2400, 513, 600])
    hf = vbx.HiFiGANMelCodec(n_fft=256, hop_size=64, win_size=256, num_mels=80)
    with pytest.raises(ValueError, match=r"HiFiGANMelCodec\.encode: lens\[0\] = 96 is outside 97 \.\. T = 2400"):
        hf.encode(w, lens=[96, 97, 2400])
    enc = vbx.SEANetEncoder(n_filters=16, ratios=(4, 2), dimension=32)
    with pytest.raises(ValueError, match=r"SEANetEncoder: lens\[0\] = 0 is outside 1 \.\. T = 2400"):
        enc(w, lens=[0, 1, 2400])
    with pytest.raises(ValueError, match=r"resample: lens\[2\] = 2401 is outside 1 \.\. T = 2400"):
        vbx.resample(w, 16000, 24000, lens=[1, 2, 2401])
    with pytest.raises(ValueError, match=r"padded batch"):
        vbx.resample(torch.zeros(2, 3, 100), 16000, 24000, lens=[1, 2])
    codec = vbx.EncodecVocoCodec(rvq=vbx.ResidualVQ(dim=32, codebook_size=64, num_quantizers=2), vocoder=None, encoder=enc)
    with pytest.raises(ValueError, match=r"EncodecVocoCodec\.encode: lens\[1\] = 0"):
        codec.encode(w, lens=[5, 0, 7])
    own = vbx.EncodecVocoCodec(rvq=vbx.ResidualVQ(dim=32, codebook_size=64, num_quantizers=2), vocoder=None,
                               encoder=torch.nn.Identity())
    with pytest.raises(NotImplementedError, match="needs an encoder with frame_lens"):
        own.encode(w, lens=[5, 6, 7])


def test_device_lens_clamps_tensors_that_are_not_on_the_host():
    """the device branch without a device: a `meta` tensor takes it (no value can be read), and comes back int32 of the same shape"""
    from voicebox_pytorch_amd.wave_lens import device_lens

    out = device_lens(torch.empty(4, dtype=torch.int64, device="meta"), 4, 100, 7, "meta", "who")
    assert out.dtype == torch.int32 and out.shape == (4,) and out.device.type == "meta"
    assert device_lens(torch.tensor([7, 100]), 2, 100, 7, "cpu", "who").tolist() == [7, 100]
    # the clamp itself, as the device branch applies it
    assert torch.tensor([0, 107, 50]).clamp(7, 100).tolist() == [7, 100, 50]


# ------------------------------------------------------------------------------------------------ wrapper / train step refusals
def _wrapper(codec=None, **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=5, depth=2, dim_head=64, heads=2, audio_enc_dec=codec,
                      condition_on_text=kw.pop("condition_on_text", False))
    return vbx, vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb, **kw)


def test_wrapper_refusals_and_messages():
    import voicebox_pytorch_amd as vbx

    _, _, w = _wrapper(vbx.LogMelCodec())
    wave, lat = torch.randn(3, 2400), torch.randn(3, 16, 100)
    with pytest.raises(ValueError, match=r"forward: wave_lens counts samples of raw audio.*x1 \(3, 16, 100\) holds latents.*lens in frames"):
        w(lat, wave_lens=[2400, 700, 600])
    with pytest.raises(ValueError, match=r"wave_lens and mask both given.*pass one of them"):
        w(wave, wave_lens=[2400, 700, 600], mask=torch.ones(3, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"wave_lens and lens both given"):
        w(lat, wave_lens=[2400, 700, 600], lens=[16, 5, 4])
    with pytest.raises(ValueError, match=r"raw audio.*encode first.*or pass mask, or pass wave_lens="):  # lens= keeps refusing waves
        w(wave, lens=[16, 5, 4])
    with pytest.raises(ValueError, match=r"LogMelCodec\.encode: lens\[1\] = 400 is outside 513 \.\. T = 2400"):
        w(wave, wave_lens=[2400, 400, 600])
    with pytest.raises(ValueError, match=r"sample: wave_lens and lens both given"):
        w.sample(cond=wave, wave_lens=[2400, 700, 600], lens=[16, 5, 4])
    with pytest.raises(ValueError, match=r"sample: wave_lens counts samples.*cond \(3, 16, 100\) holds latents"):
        w.sample(cond=lat, wave_lens=[2400, 700, 600])
    with pytest.raises(ValueError, match=r"encode_raw_audio: wave_lens counts samples"):
        w.encode_raw_audio(lat, wave_lens=[2400, 700, 600])
    # a codec that is not the row alone under lengths: what is missing is named
    _, _, wt = _wrapper(ToyCodec(64))
    with pytest.raises(ValueError, match=r"ToyCodec has no frame_lens\(sample_lens\) and `lens` in encode's signature"):
        wt(torch.randn(3, 160), wave_lens=[160, 100, 50])
    with pytest.raises(ValueError, match=r"ToyCodec has no"):
        wt.sample(cond=torch.randn(3, 160), wave_lens=[160, 100, 50])

    class HalfCodec(ToyCodec):
        def frame_lens(self, lens):
            return [l // self.hop for l in lens]

    _, _, wh = _wrapper(HalfCodec(64))
    with pytest.raises(ValueError, match=r"HalfCodec has no `lens` in encode's signature"):
        wh(torch.randn(3, 160), wave_lens=[160, 100, 50])
    _, _, wn = _wrapper(None)
    with pytest.raises(ValueError, match=r"wave_lens needs audio_enc_dec"):
        wn(torch.randn(3, 160), wave_lens=[160, 100, 50])


def test_wave_lens_refuses_ids_from_wav2vec():
    import voicebox_pytorch_amd as vbx

    class W2V:
        target_sample_hz, downsample_factor, codebook_size = 16000, 320, 5

        def __call__(self, wave):
            raise AssertionError("the refusal comes first")

    _, _, w = _wrapper(vbx.LogMelCodec(), condition_on_text=True, wav2vec=W2V())
    with pytest.raises(NotImplementedError, match=r"wave_lens with token ids from wav2vec= is not built.*pass semantic_token_ids"):
        w(torch.randn(2, 2400), wave_lens=[2400, 700])


def test_train_step_refusals_come_before_the_device():
    """TrainStep._forward_backward calls wave_lens.refuse first thing (the step object itself needs a device: the check it runs is
    exercised here with its arguments)"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import wave_lens as wl

    mel, wave = vbx.LogMelCodec(), torch.randn(2, 2400)
    wl.refuse([2400, 700], wave, None, None, None, mel, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: wave_lens and lens both given"):
        wl.refuse([2400, 700], wave, None, [16, 5], None, mel, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: wave_lens and mask both given"):
        wl.refuse([2400, 700], wave, None, None, torch.ones(2, 16, dtype=torch.bool), mel, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: wave_lens counts samples of raw audio"):
        wl.refuse([2400, 700], torch.randn(2, 16, 100), None, None, None, mel, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: .*ToyCodec has no"):
        wl.refuse([160, 100], torch.randn(2, 160), None, None, None, ToyCodec(64), "TrainStep")
    with pytest.raises(NotImplementedError, match=r"TrainStep: .*pass semantic_token_ids"):
        wl.refuse([2400, 700], wave, None, None, None, mel, "TrainStep", wav2vec_ids=True)
    import inspect
    from voicebox_pytorch_amd.dp import TrainStep

    for fn in (TrainStep.step, TrainStep.accumulate, TrainStep.accumulate_last_and_apply):
        assert "wave_lens" in inspect.signature(fn).parameters and "input_sampling_rate" in inspect.signature(fn).parameters


# ------------------------------------------------------------------------------------------------ trainer
def test_collate_lengths_reach_the_step_as_wave_lens():
    from voicebox_pytorch_amd.trainer import VoiceBoxTrainer, _collate

    _, _, w = _wrapper()
    t = VoiceBoxTrainer.__new__(VoiceBoxTrainer)
    torch.nn.Module.__init__(t)
    t.cfm_wrapper, t.input_sampling_rate, t.mask_padding, t.mask_wave_padding = w, 16000, False, True
    waves = [torch.randn(n) for n in (800, 640, 123)]
    batch = _collate(True, with_lens=True)(waves)
    xb, kw = t._model_kwargs(batch)
    assert xb.shape == (3, 800) and set(kw) == {"wave_lens", "input_sampling_rate"} and kw["wave_lens"].tolist() == [800, 640, 123]
    with pytest.raises(ValueError, match=r"mask_wave_padding=True.*waves.*mask_padding=True"):
        t._model_kwargs(_collate(True, with_lens=True)([torch.randn(n, 64) for n in (9, 4)]))
    # mask_padding keeps its meaning and its refusal of waves
    t.mask_padding, t.mask_wave_padding = True, False
    lat = _collate(True, with_lens=True)([torch.randn(n, 64) for n in (9, 4)])
    xb, kw = t._model_kwargs(lat)
    assert set(kw) == {"lens", "input_sampling_rate"} and kw["lens"].tolist() == [9, 4]
    with pytest.raises(ValueError, match=r"mask_padding=True.*latents.*codec"):
        t._model_kwargs(batch)
    t.mask_padding = False
    assert t._model_kwargs((xb,))[1] == {"input_sampling_rate": 16000}  # neither flag: nothing is added
    import inspect

    sig = inspect.signature(VoiceBoxTrainer.__init__).parameters
    assert sig["mask_wave_padding"].default is False and sig["mask_padding"].default is False


# ------------------------------------------------------------------------------------------------ AudioDataset
def _write_wav(path, samples, width=2, channels=1, rate=24000):
    path.parent.mkdir(parents=True, exist_ok=True)
    with wavelib.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        if width == 1:
            raw = bytes((s >> 8) + 128 for s in samples)
        elif width == 2:
            raw = struct.pack(f"<{len(samples)}h", *samples)
        elif width == 3:
            raw = b"".join(struct.pack("<i", s << 8)[:3] for s in samples)
        else:
            raw = struct.pack(f"<{len(samples)}i", *[s << 16 for s in samples])
        f.writeframes(raw)


def test_audio_dataset(tmp_path, monkeypatch):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import data

    monkeypatch.setattr(data, "_torchaudio", lambda: None)  # the stdlib path, whether or not torchaudio is installed
    a = [0, 1, -1, 32767, -32768, 12345, -256, 256]
    b = [100 * i - 700 for i in range(15)]
    _write_wav(tmp_path / "a.wav", a)
    _write_wav(tmp_path / "deep" / "er" / "b.wav", b)
    (tmp_path / "notes.txt").write_text("not audio")
    torch.save(torch.arange(5.0), tmp_path / "c.pt")
    ds = vbx.AudioDataset(tmp_path)
    assert len(ds) == 2 and ds.audio_extension == ".wav"  # recursion, and the extension filter
    by_len = {ds[i].numel(): ds[i] for i in range(2)}
    for ref in (a, b):
        got = by_len[len(ref)]
        assert got.dtype == torch.float32 and got.ndim == 1
        assert torch.equal(got, torch.tensor(ref, dtype=torch.float32) / 32768)
    assert torch.equal(vbx.AudioDataset(tmp_path, audio_extension=".pt")[0], torch.arange(5.0))
    # the other PCM widths: the same values at their own resolution
    for width, tol in ((1, 2 ** -7), (3, 0.0), (4, 0.0)):
        d = tmp_path / f"w{width}"
        _write_wav(d / "x.wav", a, width=width)
        got = vbx.AudioDataset(d)[0]
        assert float((got - torch.tensor(a, dtype=torch.float32) / 32768).abs().max()) <= tol, width
    # the reference's two asserts
    with pytest.raises(AssertionError, match="folder does not exist"):
        vbx.AudioDataset(tmp_path / "nowhere")
    with pytest.raises(AssertionError, match="no files found"):
        vbx.AudioDataset(tmp_path, audio_extension=".flac")
    # a stereo file and an undecodable extension raise, naming the file
    _write_wav(tmp_path / "st" / "two.wav", a, channels=2)
    with pytest.raises(RuntimeError, match=r"two\.wav.*not a mono wave"):
        vbx.AudioDataset(tmp_path / "st")[0]
    (tmp_path / "fl").mkdir()
    (tmp_path / "fl" / "x.flac").write_bytes(b"fLaC")
    with pytest.raises(RuntimeError, match=r"x\.flac.*no decoder for '\.flac'.*torchaudio is not installed"):
        vbx.AudioDataset(tmp_path / "fl", audio_extension=".flac")[0]
    # through the trainer's collate function: waves and their lengths
    from voicebox_pytorch_amd.trainer import _collate

    xb, lens = _collate(True, with_lens=True)([ds[0], ds[1]])
    assert xb.shape == (2, 15) and sorted(lens.tolist()) == [8, 15]


# ------------------------------------------------------------------------------------------------ teeth
# the restatements' own agreement with the device kernels, as recorded on an MI355X
LOGMEL_KERNEL_DB = 7.84e-5       # profiles/codec_parity.txt: logmel {} T=24000, max |dB err| kernel
CAUSAL_ENC_VS_FP64 = 2.536e-3    # profiles/seanet_causal_parity.txt: causal encoder small-r1 T 1003, max |delta| / RMS vs fp64


def test_zero_padding_moves_the_last_live_frames_far_beyond_kernel_agreement():
    """What the bit-equality tests on the device would see from a kernel that ignored the lengths: the row zero-padded to the batch
    length and then encoded, against the row alone, on its LIVE frames, in the fp64 restatements on a non-silent wave."""
    T = 2400
    sig = mel_ref.test_signal(batch=1, seconds=0.1, seed=0)  # [1, 2400]
    for l in (2399, 1600, 1599, 640, 513):
        f = 1 + l // 160
        alone = mel_ref.log_mel(sig[:, :l])
        padded = mel_ref.log_mel(torch.nn.functional.pad(sig[:, :l], (0, T - l)))[:, :f]
        assert alone.shape[1] == f
        move = float((alone - padded).abs().max())
        first = int(((alone - padded).abs().amax(dim=(0, 2)) > 0).nonzero()[0])
        print(f"PARITY logmel len {l}: zero padding moves the live frames by up to {move:.3e} dB (first moved frame {first} of {f}); "
              f"kernel vs restatement {LOGMEL_KERNEL_DB:.2e} dB")
        assert move > 100 * LOGMEL_KERNEL_DB, (l, move)
        assert first >= f - 1 - (512 + 159) // 160, (l, first)  # only frames whose window crosses the end of the row
    cfg = dict(S.SMALL, n_residual_layers=1)
    sd = S.random_state(cfg, 0)
    wave = C.wave(1, 1003, 0)
    for encode, name in ((C.encode, "causal"), (S.encode, "non-causal")):
        for l in (1003, 192, 13, 7):
            Tb = 1011
            f = S.frames(cfg, l)
            alone = encode(sd, cfg, wave[:, :l])
            padded = encode(sd, cfg, torch.nn.functional.pad(wave[:, :l], (0, Tb - l)))[:, :f]
            move = float(S.rel_err(padded, alone))
            print(f"PARITY seanet {name} len {l}: zero padding moves the live frames by {move:.3e} (max |delta| / RMS); "
                  f"kernel vs fp64 restatement {CAUSAL_ENC_VS_FP64:.3e}")
            if name == "causal" and l % 8 == 0:
                # no `extra` at any stage and nothing padded on the right: a causal row cannot see what follows it, the padding
                # moves nothing, and at such a length the device test has no teeth for this network (the other lengths have)
                assert move == 0.0, (name, l, move)
            else:
                assert move > 10 * CAUSAL_ENC_VS_FP64, (name, l, move)
