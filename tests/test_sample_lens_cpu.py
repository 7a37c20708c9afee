"""CPU (-m "not gpu"): sample(lens=, length_bucket=) -- the yardstick the GPU tests compare against, the host logic, and the
contract of the length regulator kernel as a torch restatement.

masked_sample() below is that yardstick: the reference's sampling loop (torchdiffeq's fixed-grid midpoint, euler, rk4 3/8 rule)
over oracle.restate.voicebox_forward(..., self_attn_mask=) with the semantics sample(lens=) states -- past len_b the loader writes
"masked" into cond_mask and 0 into cond, y0 is zeroed, frames n >= len_b are masked keys.  tests/test_sample_lens_gpu.py imports it."""
import pytest
import torch

from oracle import restate

import ode_ref


def masked_sample(state, cfg, y0, cond, cond_mask, lens, steps, method="midpoint", dtype=torch.float64, cond_token_ids=None,
                  cond_scale=1.0):
    """-> [B, N, D] in `dtype`; frames >= len_b are whatever the padding rows evolve to (callers compare real frames only)."""
    B, N, _ = y0.shape
    f = lambda x: x.to(dtype) if x.is_floating_point() else x
    p = {k: f(v) for k, v in state.items()}
    mask = torch.arange(N)[None] < torch.as_tensor(lens)[:, None]
    cm = torch.ones(B, N, dtype=torch.bool) if cond_mask is None else cond_mask.clone()
    cm = cm | ~mask
    cond = (cond.to(dtype) * mask[..., None])
    y0 = y0.to(dtype) * mask[..., None]

    def fn(t, y):
        def fwd(drop):
            return restate.voicebox_forward(p, cfg, y, t.to(dtype), cond, cm, self_attn_mask=mask, cond_token_ids=cond_token_ids,
                                            cond_drop_mask=drop)
        out = fwd(None)
        if cond_scale != 1.0:
            null = fwd(torch.ones(B, dtype=torch.bool))
            out = null + (out - null) * cond_scale
        return out

    with torch.no_grad():
        return ode_ref.odeint(fn, y0, torch.linspace(0, 1, steps).to(dtype), method=method)


def plant(x, lens, gen, scale=1e3):
    """a copy of x [B, N, ...] with garbage past each length: scale * randn for floats, coin flips for bools"""
    x = x.clone()
    for b, L in enumerate(lens):
        tail = x[b, L:]
        if x.dtype == torch.bool:
            tail.copy_(torch.rand(tail.shape, generator=gen) < 0.5)
        else:
            tail.copy_(scale * torch.randn(tail.shape, generator=gen))
    return x


def test_the_yardstick_is_row_independent(golden):
    """B = 3, N = 40, lens (40, 17, 1), garbage planted past every length in cond, cond_mask and y0: the real frames of every row
    equal the same row integrated ALONE at N = len_b, in fp64 to 1e-10 -- what the GPU tests compare against is well defined."""
    g = golden("small_wc")
    cfg = restate.Cfg(**g["cfg"])
    gen = torch.Generator().manual_seed(11)
    B, N, D, lens = 3, 40, g["cfg"]["dim"], (40, 17, 1)
    cond, y0 = torch.randn(B, N, D, generator=gen), torch.randn(B, N, D, generator=gen)
    cmask = torch.rand(B, N, generator=gen) < 0.6
    cond_g, y0_g, cmask_g = plant(cond, lens, gen), plant(y0, lens, gen), plant(cmask, lens, gen)
    got = masked_sample(g["state"], cfg, y0_g, cond_g, cmask_g, lens, 5)
    assert got.dtype == torch.float64
    for b, L in enumerate(lens):
        alone = masked_sample(g["state"], cfg, y0[b:b + 1, :L], cond[b:b + 1, :L], cmask[b:b + 1, :L], (L,), 5)
        # the row alone, without any mask at all: today's path
        p64 = {k: v.double() if v.is_floating_point() else v for k, v in g["state"].items()}
        fn = lambda t, y: restate.voicebox_forward(p64, cfg, y, t, cond[b:b + 1, :L].double(), cmask[b:b + 1, :L])
        with torch.no_grad():
            plain = ode_ref.odeint(fn, y0[b:b + 1, :L].double(), torch.linspace(0, 1, 5).double(), method="midpoint")
        err = float((got[b, :L] - plain[0]).abs().max())
        print("row", b, "len", L, "max |batch - alone|", err, "masked-alone vs plain-alone", float((alone - plain).abs().max()))
        assert err < 1e-10, (b, L, err)
        assert float((alone - plain).abs().max()) < 1e-10


def _cpu_wrapper():
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=5, depth=2, dim_head=64, heads=2, condition_on_text=False)
    return vbx, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def test_lens_validation_and_messages():
    from voicebox_pytorch_amd.sample_lens import validate_lens

    ok = validate_lens([40, 17, 1], 3, 40)
    assert ok.dtype == torch.int32 and ok.device.type == "cpu" and ok.tolist() == [40, 17, 1]
    assert validate_lens(torch.tensor([3, 2], dtype=torch.int16), 2, 3).tolist() == [3, 2]
    with pytest.raises(ValueError, match=r"lens\[1\] = 41 is outside 1 \.\. N = 40"):
        validate_lens([40, 41, 1], 3, 40)
    with pytest.raises(ValueError, match=r"lens\[2\] = -1"):
        validate_lens([40, 4, -1], 3, 40)
    with pytest.raises(ValueError, match=r"lens\[0\] = 0: a row without frames has no sample"):
        validate_lens(torch.tensor([0, 4, 5]), 3, 40)
    with pytest.raises(ValueError, match="one entry per batch row"):
        validate_lens([40, 4], 3, 40)
    with pytest.raises(ValueError, match="int tensor"):
        validate_lens(torch.tensor([1.0, 2.0, 3.0]), 3, 40)
    with pytest.raises(ValueError, match="ints"):
        validate_lens([1.5, 2, 3], 3, 40)
    # through the public entry point: the values are checked before anything is built
    vbx, w = _cpu_wrapper()
    cond = torch.randn(3, 40, 64)
    with pytest.raises(ValueError, match=r"lens\[1\] = 41"):
        w.sample(cond=cond, steps=3, lens=[40, 41, 1])
    with pytest.raises(ValueError, match="a row without frames has no sample"):
        w.sample(cond=cond, steps=3, lens=[40, 0, 1])


def test_bucket_arithmetic_and_refusals():
    from voicebox_pytorch_amd.sample_lens import bucketed, pad_frames

    assert [bucketed(n, 64) for n in (1, 64, 65)] == [64, 64, 128]
    assert bucketed(65, None) == 65 and bucketed(65, 1) == 65 and bucketed(130, 64) == bucketed(190, 64) == 192
    for bad in (0, -64, 1.5, True):
        with pytest.raises(ValueError, match="length_bucket must be an int >= 1"):
            bucketed(65, bad)
    cond, y0 = torch.randn(2, 5, 4), torch.randn(2, 5, 4)
    c, y, m, ids = pad_frames(8, cond, y0, torch.zeros(2, 5, dtype=torch.bool), torch.full((2, 5), 7))
    assert c.shape == y.shape == (2, 8, 4) and torch.equal(c[:, :5], cond) and not c[:, 5:].any() and not y[:, 5:].any()
    assert m.shape == (2, 8) and m[:, 5:].all() and not m[:, :5].any() and ids.shape == (2, 8) and not ids[:, 5:].any()
    assert pad_frames(8, cond, y0, None, None)[2:] == (None, None)
    vbx, w = _cpu_wrapper()
    with pytest.raises(ValueError, match="length_bucket needs lens"):
        w.sample(cond=cond.expand(2, 5, 4), steps=3, length_bucket=64)


def test_lens_durations_needs_the_phoneme_path():
    import voicebox_pytorch_amd as vbx

    _, w = _cpu_wrapper()
    with pytest.raises(ValueError, match="'durations'"):
        w.sample(cond=torch.randn(2, 8, 64), steps=3, lens="durations")
    vb = vbx.VoiceBox(dim=64, num_cond_tokens=37, depth=2, dim_head=64, heads=2, dim_cond_emb=48, condition_on_text=True)
    wt = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)  # text-conditioned, but no duration predictor
    with pytest.raises(ValueError, match="duration_predictor"):
        wt.sample(cond=torch.randn(2, 8, 64), phoneme_ids=torch.zeros(2, 3, dtype=torch.long), steps=3, lens="durations")
    with pytest.raises(ValueError, match="'durations'"):
        wt.sample(cond=torch.randn(2, 8, 64), semantic_token_ids=torch.zeros(2, 8, dtype=torch.long), steps=3, lens="lengths")


def test_cpu_tensor_refusal_is_unchanged():
    """valid lens on a CPU model: the same refusal as without lens -- there is no CPU fallback"""
    from voicebox_pytorch_amd import _lib

    _, w = _cpu_wrapper()
    cond = torch.randn(2, 8, 64)
    with pytest.raises((_lib.VbxError, RuntimeError, AssertionError)) as plain:
        w.sample(cond=cond, steps=3)
    with pytest.raises((_lib.VbxError, RuntimeError, AssertionError)) as masked:
        w.sample(cond=cond, steps=3, lens=[8, 3], length_bucket=64)
    assert type(masked.value) is type(plain.value) and not isinstance(masked.value, ValueError)
    assert w.last_sample_lens is None


def test_length_regulator_contract_against_the_aligner_helper():
    """vbx_length_regulate's contract (sample_lens.length_regulate_restated) against DurationPredictor's
    align_phoneme_ids_with_durations (restated in oracle/restate.py): equal on rows without -1 padding phonemes; on rows with them
    the helper's result is the regulator's followed by the padding phonemes' frames (id -1), nothing else."""
    from voicebox_pytorch_amd.sample_lens import length_regulate_restated

    ids = torch.tensor([[5, 9, 3, 7, 2], [4, 6, 8, -1, -1], [1, -1, -1, -1, -1]])
    dur = torch.tensor([[0.2, 1.0, 1.99, 7.5, -3.0], [7.5, 0.2, 1.99, 1.0, 7.5], [1.99, -2.0, 0.2, 7.5, 1.0]])
    got, lens = length_regulate_restated(ids, dur)
    want = restate.align_phoneme_ids_with_durations(ids, dur)
    reps = dur.clamp(min=1).int()
    assert reps.tolist() == [[1, 1, 1, 7, 1], [7, 1, 1, 1, 7], [1, 1, 1, 7, 1]]
    assert lens.tolist() == [11, 9, 1] and got.shape == (3, 11) and got.dtype == torch.int64
    assert torch.equal(got[0], want[0, :11])  # no padding phonemes: the same row
    assert got[0].tolist() == [5, 9, 3] + [7] * 7 + [2]
    for b in (1, 2):
        L, extra = int(lens[b]), int(reps[b][ids[b] == -1].sum())
        assert torch.equal(got[b, :L], want[b, :L]) and not got[b, L:].any()
        assert (want[b, L:L + extra] == -1).all() and not want[b, L + extra:].any()  # the difference: exactly those frames
    assert want.shape[1] == 17  # the helper sizes the batch by a row of padding frames (row 1: 9 + 8)
    # one row, negative and fractional durations only
    one, l1 = length_regulate_restated(torch.tensor([[3, 4]]), torch.tensor([[-5.0, 0.2]]))
    assert one.tolist() == [[3, 4]] and l1.tolist() == [2]
