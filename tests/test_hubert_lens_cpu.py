"""Host side of HubertWithKmeans(wave, lens=) and of token_lens=, and the TEETH of tests/test_hubert_lens_gpu.py.

The restatement with lengths (tests/hubert_lens_ref.py) is held to hubert_ref.features of each row alone; each planted partial fault
-- statistics over the whole padded row, the positional convolution reading what lies past the row, attention over all keys -- is
measured on the live frames, beside what today's lens=None gives on the zero-padded batch; the figures go to
profiles/hubert_lens_parity.txt and set the tolerance of the GPU feature tests.  Then frame_lens, the validation messages,
seq_len_multiple_of, wav2vec_lacks and every new refusal, all of which arrive before a device is needed."""
import os

import pytest
import torch

import hubert_lens_ref as LR
import hubert_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement and its teeth
@pytest.mark.parametrize("T,lens", [(5000, (5000, 3333, 1285, 719)), (5000, (400, 720, 721, 4999)), (9040, (9040, 8720, 400))])
def test_restatement_with_lens_is_each_row_alone(T, lens):
    sd, wave = R.small_state_dict(), R.make_wave(len(lens), T, 5 + T % 7)
    with torch.no_grad():
        got = LR.features_lens(sd, R.SMALL, wave, lens, 4)
        alone = LR.rows_alone(sd, R.SMALL, wave, lens, 4)
        noise = wave.clone()
        for b, l in enumerate(lens):
            noise[b, l:] = 7.0 * torch.randn(T - l, generator=torch.Generator().manual_seed(b))
        again = LR.features_lens(sd, R.SMALL, noise, lens, 4)
    for b, a in enumerate(alone):
        f = a.shape[0]
        assert f == LR.frame_lens(lens, R.SMALL)[b]
        err = float((got[b, :f] - a).abs().max())
        assert err < 1e-12, (b, err)
        assert (got[b, f:] == 0).all()
    assert float((again - got).abs().max()) < 1e-12  # the padding's content moves nothing


def test_partial_faults_move_the_live_frames_and_set_the_tolerance():
    tol, table = LR.tolerance_lens()
    small, _ = R.tolerance_small()
    c = LR.LENS_CASE
    lines = ["HubertWithKmeans(lens=): what a kernel that forgets ONE of the length rules does to the live frames (tests/hubert_lens_ref.py)",
             f"fp64 restatement, SMALL, layer {c['layer']}, non-silent make_wave rows, lengths {list(c['lens'])} in a batch of {c['T']} samples;",
             "movement = max over the rows of max |delta| / RMS against the row alone, live frames only", ""]
    for f in LR.LENS_FAULTS:
        lines.append(f"PARITY fault {f:<18} moves the live frames by {table[f]:.3e}")
    lines.append(f"PARITY zero_padded_batch   (lens=None on the zero-padded batch: all of them) {table['zero_padded_batch']:.3e}")
    lines.append(f"PARITY tolerance_small() {small:.3e}; tolerance under lengths = min(that, smallest partial fault / 10) = {tol:.3e}")
    text = "\n".join(lines) + "\n"
    print(text)
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "hubert_lens_parity.txt"), "w") as fh:
            fh.write(text)
    except OSError:
        pass  # a read-only checkout: the figures are in the output above
    assert tol == min(small, min(table[f] for f in LR.LENS_FAULTS) / 10.0) and tol > 0
    for f in LR.LENS_FAULTS:
        assert table[f] > 10 * 2.0 ** -11, (f, table[f])  # each fault is far above what an fp16 rounding resolves
    assert table["zero_padded_batch"] > 1.0  # today's answer on a padded batch is another signal's


# ------------------------------------------------------------------------------------------------ host logic of HubertWithKmeans
def _small(**kw):
    import voicebox_pytorch_amd as vbx

    return vbx.HubertWithKmeans(**R.SMALL, output_layer=4, codebook_size=64, **kw)


def test_frame_lens_is_the_conv_chain():
    m = _small()
    assert m.min_samples() == 400 == LR.min_samples(R.SMALL)
    lens = list(range(400, 1400)) + [5000, 16000, 41360]
    want = [R.frames_of(l, R.SMALL) for l in lens]
    assert m.frame_lens(lens) == want == [m.frames(l) for l in lens]
    t = m.frame_lens(torch.tensor(lens))
    assert t.dtype == torch.int64 and t.tolist() == want
    assert m.frame_lens(torch.tensor(lens, dtype=torch.int32)).dtype == torch.int32
    assert m.frame_lens([400, 719, 720, 20560, 20880]) == [1, 1, 2, 64, 65]
    mm = _small(seq_len_multiple_of=320)
    assert mm.frame_lens(lens) == [R.frames_of(l // 320 * 320, R.SMALL) for l in lens]
    with pytest.raises(ValueError, match="must hold ints"):
        m.frame_lens([400.0])


def test_lengths_are_validated_on_the_host_and_name_the_row():
    """a list or a CPU tensor: ValueError naming the row, before the device is asked for"""
    import voicebox_pytorch_amd as vbx

    m, w = _small(), torch.zeros(3, 5000)
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[1\] = 399 is outside 400 \.\. T = 5000"):
        m(w, lens=[5000, 399, 400])
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[2\] = 5001 is outside 400 \.\. T = 5000"):
        m.features(w, lens=torch.tensor([5000, 400, 5001]))
    with pytest.raises(ValueError, match="one entry per batch row"):
        m(w, lens=[5000, 400])
    with pytest.raises(ValueError, match="int tensor"):
        m(w, lens=torch.tensor([5000., 400., 400.]))
    with pytest.raises(vbx._lib.VbxError, match="runs only on an MI355X"):  # valid lengths: the next check is the device
        m(w, lens=[5000, 400, 719])
    with pytest.raises(NotImplementedError, match="mask"):  # attention_mask= keeps raising, lengths or not
        m(w, attention_mask=torch.ones(3, 5000), lens=[5000, 400, 719])
    # at another rate the lengths are checked at the rate they are given in, then at the target rate: 599 samples at 24 kHz are 400
    # at 16 kHz (one frame), 598 are 399
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[0\] = 5001 is outside 1 \.\. T = 5000"):
        m(w, input_sample_hz=24000, lens=[5001, 600, 600])
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[1\] = 399 is outside 400 \.\. T = 3334"):
        m(w, input_sample_hz=24000, lens=[5000, 598, 600])
    with pytest.raises(vbx._lib.VbxError, match="runs only on an MI355X"):
        m(w, input_sample_hz=24000, lens=[5000, 599, 600])
    # seq_len_multiple_of floors each length as the wave is curtailed: 719 -> 640 is a frame, 639 -> 320 is none
    mm = _small(seq_len_multiple_of=320)
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[1\] = 320 is outside 400 \.\. T = 4800"):
        mm(w, lens=[5000, 639, 719])
    with pytest.raises(vbx._lib.VbxError, match="runs only on an MI355X"):
        mm(w, lens=[5000, 640, 719])
    with pytest.raises(NotImplementedError, match="shorter than one frame"):
        m(torch.zeros(2, 399), lens=[399, 399])


def test_signatures():
    import inspect

    import voicebox_pytorch_amd as vbx

    H = vbx.HubertWithKmeans
    assert list(inspect.signature(H.forward).parameters) == ["self", "wav_input", "flatten", "input_sample_hz", "attention_mask", "lens"]
    assert inspect.signature(H.forward).parameters["lens"].default is None
    assert inspect.signature(H.features).parameters["lens"].default is None
    assert callable(H.frame_lens)


# ------------------------------------------------------------------------------------------------ wav2vec_lacks and the refusals
class _NoLens:
    target_sample_hz, downsample_factor, codebook_size = 16000, 320, 5

    def __call__(self, wave):
        raise AssertionError("the refusal comes first")


class _HalfLens(_NoLens):
    def __call__(self, wave, lens=None):
        raise AssertionError("the refusal comes first")


def test_wav2vec_lacks_names_what_is_missing():
    from voicebox_pytorch_amd import wave_lens as wl

    assert wl.wav2vec_lacks(_small()) is None
    assert wl.wav2vec_lacks(_NoLens()) == "`lens` in its call signature and frame_lens(sample_lens)"
    assert wl.wav2vec_lacks(_HalfLens()) == "frame_lens(sample_lens)"
    assert wl.wav2vec_lacks(torch.nn.Identity()) == "`lens` in its call signature and frame_lens(sample_lens)"


def _wrapper(codec=None, **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=5, depth=2, dim_head=64, heads=2, audio_enc_dec=codec,
                      condition_on_text=kw.pop("condition_on_text", True), dim_cond_emb=64)
    return vbx, vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb, **kw)


def test_refusal_of_a_wav2vec_without_lengths_names_what_is_missing():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import wave_lens as wl

    wave = torch.randn(2, 2400)
    for w2v, what in ((_NoLens(), r"_NoLens has no `lens` in its call signature and frame_lens"), (_HalfLens(), r"_HalfLens has no frame_lens")):
        _, _, w = _wrapper(vbx.LogMelCodec(), wav2vec=w2v)
        with pytest.raises(NotImplementedError, match=r"wave_lens with token ids from wav2vec= is not built.*" + what + r".*pass semantic_token_ids"):
            w(wave, wave_lens=[2400, 700])
        with pytest.raises(NotImplementedError, match=r"wav2vec_token_ids: wave_lens needs a wav2vec.*has no"):
            w.wav2vec_token_ids(wave, None, wave_lens=[2400, 700])
    # refuse() called directly keeps raising, with or without the object
    with pytest.raises(NotImplementedError, match=r"TrainStep: wave_lens with token ids from wav2vec= is not built.*pass semantic_token_ids"):
        wl.refuse([2400, 700], wave, None, None, None, vbx.LogMelCodec(), "TrainStep", wav2vec_ids=True)
    # a wav2vec that serves lengths is not refused: the next thing in the way is the codec's own validation, then the device
    _, _, w = _wrapper(vbx.LogMelCodec(), wav2vec=_small())
    wl.refuse([2400, 700], wave, None, None, None, vbx.LogMelCodec(), "forward", wav2vec_ids=False, wav2vec=_small())
    with pytest.raises(vbx._lib.VbxError, match=r"runs only on an MI355X"):  # 2400 and 700 samples at 24 kHz are valid for both
        w(wave, wave_lens=[2400, 700])
    # a CPU tensor is validated on the host like a list, naming the row -- by resample where the rates differ, by the wav2vec itself
    # where they do not (399 samples at 16 kHz are short of one frame)
    with pytest.raises(ValueError, match=r"resample: lens\[0\] = 2401 is outside 1 \.\. T = 2400"):
        w.wav2vec_token_ids(wave, None, wave_lens=torch.tensor([2401, 700]))
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[1\] = 399 is outside 400 \.\. T = 2400"):
        w.wav2vec_token_ids(wave, 16000, wave_lens=torch.tensor([2400, 399]))
    with pytest.raises(ValueError, match=r"resample: lens\[1\] = 0 is outside 1 \.\. T = 2400"):
        w(wave, wave_lens=torch.tensor([2400, 0]))
    # ids given: wav2vec= is not asked, whatever it lacks
    _, _, w = _wrapper(vbx.LogMelCodec(), wav2vec=_NoLens())
    with pytest.raises(vbx._lib.VbxError, match="runs only on an MI355X"):
        w(wave, wave_lens=[2400, 700], semantic_token_ids=torch.zeros(2, 5, dtype=torch.long))


def test_token_lens_refusals_come_before_the_device():
    import inspect

    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import wave_lens as wl
    from voicebox_pytorch_amd.dp import TrainStep

    _, vb, w = _wrapper()
    lat, ids = torch.randn(2, 16, 64), torch.zeros(2, 5, dtype=torch.long)
    who = r"ConditionalFlowMatcherWrapper\.forward"
    with pytest.raises(ValueError, match=who + r": token_lens resizes row b's ids to row b's own frames.*lens="):
        w(lat, semantic_token_ids=ids, token_lens=[5, 3])
    with pytest.raises(ValueError, match=who + r": token_lens counts the token ids of each row, and no token ids were given"):
        w(lat, lens=[16, 9], token_lens=[5, 3])
    with pytest.raises(ValueError, match=who + r": token_lens with phoneme_ids"):
        w(lat, lens=[16, 9], phoneme_ids=ids, token_lens=[5, 3])
    with pytest.raises(ValueError, match=who + r": token_lens\[1\] = 6 is outside 1 \.\. T = 5"):
        w(lat, lens=[16, 9], semantic_token_ids=ids, token_lens=[5, 6])
    with pytest.raises(ValueError, match=who + r": token_lens\[0\] = 0 is outside 1 \.\. T = 5"):
        w(lat, lens=[16, 9], semantic_token_ids=ids, token_lens=torch.tensor([0, 5]))
    with pytest.raises(ValueError, match="token_lens must have one entry per batch row"):
        w(lat, lens=[16, 9], semantic_token_ids=ids, token_lens=[5])
    with pytest.raises(ValueError, match=r"VoiceBox\.forward: cond_token_lens resizes.*lens="):
        vb(lat, times=torch.zeros(2), cond_token_ids=ids, cond=lat, cond_token_lens=[5, 3])
    with pytest.raises(ValueError, match=r"VoiceBox\.forward: cond_token_lens\[1\] = 9 is outside 1 \.\. T = 5"):
        vb(lat, times=torch.zeros(2), cond_token_ids=ids, cond=lat, self_attn_lens=[16, 9], cond_token_lens=[5, 9])
    with vbx.precise_mode():
        with pytest.raises(NotImplementedError, match="token_lens is not served in precise mode"):
            w(lat, lens=[16, 9], semantic_token_ids=ids, token_lens=[5, 3])
        with pytest.raises(NotImplementedError, match="cond_token_lens is not served in precise mode"):
            vb(lat, times=torch.zeros(2), cond_token_ids=ids, cond=lat, self_attn_lens=[16, 9], cond_token_lens=[5, 3])
    # TrainStep runs the same checks first thing (the step object itself needs a device)
    wl.refuse_token_lens(None, False, None, None, "TrainStep")
    wl.refuse_token_lens([5, 3], True, ids, None, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: token_lens resizes"):
        wl.refuse_token_lens([5, 3], False, ids, None, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: token_lens counts the token ids"):
        wl.refuse_token_lens([5, 3], True, None, None, "TrainStep")
    with pytest.raises(ValueError, match=r"TrainStep: token_lens with phoneme_ids"):
        wl.refuse_token_lens([5, 3], True, ids, ids, "TrainStep")
    for fn in (TrainStep.step, TrainStep.accumulate, TrainStep.accumulate_last_and_apply):
        assert inspect.signature(fn).parameters["token_lens"].default is None
    assert inspect.signature(vbx.VoiceBox.forward).parameters["cond_token_lens"].default is None
    assert inspect.signature(vbx.ConditionalFlowMatcherWrapper.forward).parameters["token_lens"].default is None
    assert "wave_lens" in inspect.signature(vbx.ConditionalFlowMatcherWrapper.wav2vec_token_ids).parameters
