"""sample(lens=, length_bucket=) on the device: batches of unequal lengths.  The yardstick is tests/test_sample_lens_cpu.py's
masked_sample (the reference's loop over oracle.restate.voicebox_forward(self_attn_mask=), shown row-independent there); weights are
the small_wc golden's (dim 64, depth 2, the well-conditioned network), inputs seeded here.  Every line that starts with PARITY is a
measured figure (profiles/sample_lens_parity.txt is those lines of one run)."""
import importlib.util
import json
import os

import pytest
import torch

from oracle import restate
from test_sample_lens_cpu import masked_sample, plant

pytestmark = pytest.mark.gpu
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
B, N, STEPS = 4, 200, 5
# R = 16 register tokens come first: R + len hits 63, 64, 65, 128, 129 and R + N = 216 over the two sets
LENS = [(200, 47, 48, 49), (112, 113, 200, 49)]
_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _golden():
    return cached("g", lambda: torch.load(os.path.join(HERE, "golden", "small_wc.pt"), map_location="cpu", weights_only=False))


def _vb():
    def build():
        import voicebox_pytorch_amd as vbx

        g = _golden()
        vb = vbx.VoiceBox(dim=g["cfg"]["dim"], num_cond_tokens=500, depth=g["cfg"]["depth"], dim_head=64, heads=g["cfg"]["heads"],
                          condition_on_text=False)
        vb.load_state_dict(g["state"], strict=False)
        vb = vb.to(dev).eval()
        assert vb._cfg["R"] == 16
        return vb
    return cached("vb", build)


def _wrapper(method="midpoint"):
    import voicebox_pytorch_amd as vbx

    return vbx.ConditionalFlowMatcherWrapper(voicebox=_vb(), torchdiffeq_ode_method=method)


def _inputs(n=N, b=B, seed=21):
    def build():
        gen = torch.Generator().manual_seed(seed)
        D = _golden()["cfg"]["dim"]
        return (torch.randn(b, n, D, generator=gen), torch.randn(b, n, D, generator=gen), torch.rand(b, n, generator=gen) < 0.6)
    return cached(("in", n, b, seed), build)  # cond, y0, cond_mask (CPU)


def _reference(method, li):
    def build():
        g = _golden()
        cond, y0, cmask = _inputs()
        return masked_sample(g["state"], restate.Cfg(**g["cfg"]), y0, cond, cmask, LENS[li], STEPS, method=method, dtype=torch.float32)
    return cached(("ref", method, li), build)


def _sample(wrapper, cond, y0, cmask, lens, **kw):
    from voicebox_pytorch_amd.masks import rng_override

    with rng_override(y0=y0):
        return wrapper.sample(cond=cond.to(dev), cond_mask=cmask.to(dev), steps=STEPS, lens=lens, **kw)


def _row_errors(out, ref, lens):
    return [rel(out[b, :L], ref[b, :L]) for b, L in enumerate(lens)]


# ------------------------------------------------------------------------------------------------ 4: against the restatement
@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("split", ["1", "2"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("method", ["midpoint", "euler", "rk4"])
def test_masked_sample_matches_the_restatement(method, use_graph, split, li, monkeypatch):
    """Real frames of every row within 2e-3 relative L2 of the fp32 restatement loop -- the bound test_well_conditioned_sampler_is_tight
    holds this network to (it measures 3 - 6e-4) -- and padding frames exactly 0: all fixed-grid methods, eager and captured, one
    stream and two concurrent half batches."""
    monkeypatch.setenv("VBX_SAMPLE_SPLIT", split)
    lens = LENS[li]
    cond, y0, cmask = _inputs()
    w = _wrapper(method)
    out = _sample(w, cond, y0, cmask, list(lens), use_graph=use_graph)
    smp = next(iter(w._samplers.values()))
    assert smp.masked and smp.split == int(split) and out.shape == (B, N, cond.shape[-1])
    assert w.last_sample_lens.dtype == torch.int64 and w.last_sample_lens.tolist() == list(lens)
    errs = _row_errors(out, _reference(method, li), lens)
    _cache[("err", method, use_graph, split, li)] = errs
    print(f"PARITY restatement {method} {'graph' if use_graph else 'eager'} split {split} lens {lens}: rel L2 per row",
          " ".join(f"{e:.2e}" for e in errs))
    for b, L in enumerate(lens):
        assert not out[b, L:].any(), (b, L)
        assert torch.equal(out[b, L:], torch.zeros_like(out[b, L:]))
    assert max(errs) < 2e-3, errs
    if use_graph:  # a second call replays the captured graph on fresh inputs
        assert torch.equal(_sample(w, cond, y0, cmask, list(lens), use_graph=True), out)


# ------------------------------------------------------------------------------------------------ 5: padding cannot leak
@pytest.mark.parametrize("method", ["midpoint", "euler", "rk4", "dopri5"])
def test_padding_cannot_leak_bit_for_bit(method):
    """The same call twice, the second with garbage (1e3 randn, coin flips) past the lengths in cond, cond_mask and the y0 override:
    real frames bit-equal, padding 0 -- any kernel that reads a padding frame into a real one fails this.  dopri5: the step counts too
    (its error norm must not see the padding)."""
    lens = LENS[0]
    cond, y0, cmask = _inputs()
    gen = torch.Generator().manual_seed(77)
    w = _wrapper(method)
    a = _sample(w, cond, y0, cmask, list(lens))
    sa = dict(w.last_sample_stats)
    b = _sample(w, plant(cond, lens, gen), plant(y0, lens, gen), plant(cmask, lens, gen), torch.tensor(lens, device=dev))
    sb = dict(w.last_sample_stats)
    assert len(w._samplers) == 1
    assert same_bits(a, b), float((a - b).abs().max())
    assert sa == sb and sa["method"] == method, (sa, sb)
    for r, L in enumerate(lens):
        assert not a[r, L:].any() and a[r, :L].abs().sum() > 0
    if method == "dopri5":
        print("PARITY dopri5 under lens", sa)


# ------------------------------------------------------------------------------------------------ 6: the attention kernel
@pytest.mark.parametrize("Np", [216, 272])
def test_attn_fwd_lens_equals_attn_fwd_with_the_prefix_mask(Np):
    """vbx_attn_fwd_lens against vbx_attn_fwd with the prefix mask through the C ABI: every live query row (fp16 and bf16 output)
    and lse bit-equal; a query tile wholly past the length holds zeros and lse 1e30; all rows full: bit-equal everywhere.  Np 216 ends
    in a full-role tail tile (88 rows), 272 in the <= 16-row ragged role.  Buffers are NaN-filled with a guard row."""
    from voicebox_pytorch_amd import _lib as L

    Bq, H, I = 3, 2, 128
    gen = torch.Generator().manual_seed(Np)
    q, k, v = ((torch.randn(Bq, H, Np, 64, generator=gen) * s).half().to(dev) for s in (1.5, 1.0, 1.0))
    nans = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=dev)

    def run(name, klens):
        kl = torch.tensor(klens, dtype=torch.int32, device=dev)
        mask = (torch.arange(Np, device=dev)[None] < kl[:, None]).contiguous()
        o16, ob, lse = nans((Bq * Np + 1, I), torch.float16), nans((Bq * Np + 1, I), torch.bfloat16), nans((Bq * H * Np + 1,), torch.float32)
        if name == "vbx_attn_fwd":
            L.call(name, q, k, v, mask, o16, ob, lse, Bq, H, Np, 10.0, _st())
        else:
            L.call(name, q, k, v, mask, kl, o16, ob, lse, Bq, H, Np, 10.0, _st())
        torch.cuda.synchronize()
        assert o16[-1].isnan().all() and ob[-1].isnan().all() and lse[-1].isnan()  # nothing past the end
        return o16[:-1].view(Bq, Np, I), ob[:-1].view(Bq, Np, I), lse[:-1].view(Bq, H, Np)

    for klens in ((1, 63, 64), (65, 128, 129), (Np - 1, Np, 1), (Np, Np, Np)):
        want, got = run("vbx_attn_fwd", klens), run("vbx_attn_fwd_lens", klens)
        assert not any(t.isnan().any() for t in got), klens
        for b, kl in enumerate(klens):
            assert same_bits(got[0][b, :kl], want[0][b, :kl]) and same_bits(got[1][b, :kl], want[1][b, :kl]), (klens, b)
            assert same_bits(got[2][b, :, :kl], want[2][b, :, :kl]), (klens, b)
            dead0 = -(-kl // 128) * 128  # the first query tile wholly past the length
            assert not got[0][b, dead0:].any() and not got[1][b, dead0:].float().any() and (got[2][b, :, dead0:] == 1e30).all()
        if klens == (Np, Np, Np):
            assert all(same_bits(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ 7: the error norm
def test_ode_norm_lens():
    """vbx_ode_norm_lens: the bits of vbx_ode_norm at full lengths (and with lens NULL) in all three modes; at short lengths the
    error ratio within (n + 2) 2^-53 of an fp64 torch sum over the kept elements (the fp32 per-element terms restated in torch),
    INIT0's d1 / h0 at fp32 accuracy; NaNs in the dropped elements change nothing."""
    from voicebox_pytorch_amd import _lib as L
    from voicebox_pytorch_amd import solver as S

    Bn, Nn, D = 3, 37, 12
    n = Bn * Nn * D
    gen = torch.Generator().manual_seed(9)
    y0, y1 = (torch.randn(Bn, Nn, D, generator=gen).to(dev) for _ in range(2))
    ks = [(torch.randn(Bn, Nn, D, generator=gen) * 1e-3).to(dev) for _ in range(7)]
    slab = torch.zeros(L.lib().vbx_ode_norm_slab_doubles(n), dtype=torch.float64, device=dev)

    def run(mode, lens, plain=False, ys=(y0, y1), kk=ks):
        state = torch.zeros(S.DP_STATE, dtype=torch.float64)
        state[S.DP_TEND], state[S.DP_ATOL], state[S.DP_RTOL], state[S.DP_DT], state[S.DP_H0], state[S.DP_D1] = 1.0, 1e-5, 1e-5, 1.0, 0.01, 0.5
        state = state.to(dev)
        S_, c = {S.NORM_ERROR: (7, S._floats(S.DP_C_ERROR)), S.NORM_INIT0: (1, None), S.NORM_INIT1: (2, None)}[mode]
        y1_ = ys[1] if mode == S.NORM_ERROR else None
        if plain:
            L.call("vbx_ode_norm", state, slab, mode, ys[0], y1_, S._ptrs(kk[:S_]), c, S_, n, 1, _st())
        else:
            ld = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
            L.call("vbx_ode_norm_lens", state, slab, mode, ys[0], y1_, S._ptrs(kk[:S_]), c, S_, n, 1, ld, Bn, D, _st())
        return state.cpu()

    for mode in (S.NORM_ERROR, S.NORM_INIT0, S.NORM_INIT1):
        want = run(mode, None, plain=True)
        assert same_bits(run(mode, (Nn,) * Bn), want) and same_bits(run(mode, None), want), mode
    lens = (37, 5, 1)
    keep = (torch.arange(Nn)[None] < torch.tensor(lens)[:, None]).to(dev)
    nk = int(keep.sum()) * D
    # ERROR: e = sum_j (c_j dt) k_j in stage order, fp32, dt = 1; q = e / (atol + rtol max(|y0|, |y1|)); ratio = sqrt(sum q^2 / n)
    e = ks[0] * S.DP_C_ERROR[0]
    for j in range(1, 7):
        e = e + ks[j] * S.DP_C_ERROR[j]
    atol = torch.tensor(1e-5, dtype=torch.float32, device=dev)
    q = e / (atol + atol * torch.maximum(y0.abs(), y1.abs()))
    ref = float(((q.double() ** 2)[keep].sum() / nk).sqrt())
    got = run(S.NORM_ERROR, lens)
    ratio = float(got[S.DP_RATIO])
    print("PARITY ode_norm_lens error ratio", ratio, "fp64 torch", ref, "rel", abs(ratio - ref) / ref, "bound", (nk + 2) * 2.0 ** -53)
    assert abs(ratio - ref) <= (nk + 2) * 2.0 ** -53 * ref
    assert got[S.DP_NFE] == 6 and got[S.DP_REJECTED] + got[S.DP_ACCEPTED] == 1
    # INIT0: d0 = rms(y0 / scale), d1 = rms(f0 / scale) over the kept elements, h0 = 0.01 d0 / d1 (fp32)
    scale = atol + y0.abs() * atol
    d0 = float((((y0 / scale).double() ** 2)[keep].sum() / nk).sqrt())
    d1 = float((((ks[0] / scale).double() ** 2)[keep].sum() / nk).sqrt())
    g0 = run(S.NORM_INIT0, lens)
    assert abs(float(g0[S.DP_D1]) - d1) < 1e-6 * d1 and abs(float(g0[S.DP_H0]) - 0.01 * d0 / d1) < 1e-6 * 0.01 * d0 / d1
    # garbage in the dropped elements (NaN: it would poison any sum it entered) changes nothing, in every mode
    drop = ~keep[..., None].expand(Bn, Nn, D)
    bad = lambda t: torch.where(drop, torch.full_like(t, float("nan")), t)
    for mode in (S.NORM_ERROR, S.NORM_INIT0, S.NORM_INIT1):
        assert same_bits(run(mode, lens, ys=(bad(y0), bad(y1)), kk=[bad(k) for k in ks]), run(mode, lens)), mode
    # vbx_zero_tail_rows
    x = torch.randn(Bn, Nn, D, device=dev)
    z = x.clone()
    L.call("vbx_zero_tail_rows", z, torch.tensor(lens, dtype=torch.int32, device=dev), Bn, Nn, D, _st())
    assert torch.equal(z, x * keep[..., None])


# ------------------------------------------------------------------------------------------------ 8: the row alone
def test_masked_row_equals_the_row_alone():
    """Row b of a masked B = 4 midpoint call on its real frames against sample() of that row by itself at N = len_b (today's path).
    Tolerance: the larger of twice the distance between two existing-path runs of the row that differ only in batch position and the
    distance of the masked call to the restatement (test 4's figure for that row) -- both are rounding, not a third error source."""
    from voicebox_pytorch_amd.masks import rng_override

    lens = LENS[0]
    cond, y0, cmask = _inputs()
    w = _wrapper()
    out = _sample(w, cond, y0, cmask, list(lens))
    to_ref = _row_errors(out, _reference("midpoint", 0), lens)
    for b, L in enumerate(lens):
        c1, y1, m1 = cond[b:b + 1, :L], y0[b:b + 1, :L], cmask[b:b + 1, :L]
        o = (b + 1) % B  # a filler row in front, cut to the same length
        c2, y2, m2 = torch.cat([cond[o:o + 1, :L], c1]), torch.cat([y0[o:o + 1, :L], y1]), torch.cat([cmask[o:o + 1, :L], m1])
        plain = _wrapper()
        with rng_override(y0=y1):
            alone = plain.sample(cond=c1.to(dev), cond_mask=m1.to(dev), steps=STEPS)
        with rng_override(y0=y2):
            second = plain.sample(cond=c2.to(dev), cond_mask=m2.to(dev), steps=STEPS)[1:]
        position, d = rel(second, alone), rel(out[b:b + 1, :L], alone)
        tol = max(2 * position, to_ref[b])
        print(f"PARITY row alone: row {b} len {L}: masked-in-batch vs alone {d:.2e}; alone at batch position 0 vs 1 {position:.2e}; "
              f"masked-in-batch vs restatement {to_ref[b]:.2e}; tolerance {tol:.2e}")
        assert d <= tol, (b, L, d, tol)


# ------------------------------------------------------------------------------------------------ 9: buckets
def test_length_bucket_shares_one_sampler():
    """N = 130 and N = 190 at length_bucket 64 run at 192 frames: one _samplers entry, the same sampler object (and its graph), and
    the real frames of the unbucketed masked calls bit for bit."""
    w, wu = _wrapper(), _wrapper()
    seen = []
    for n, lens in ((130, [130, 100, 47, 5]), (190, [64, 190, 129, 1])):
        cond, y0, cmask = _inputs(n=n, seed=n)
        got = _sample(w, cond, y0, cmask, lens, length_bucket=64)
        assert got.shape == (B, n, cond.shape[-1]) and len(w._samplers) == 1
        smp = next(iter(w._samplers.values()))
        seen.append((smp, smp.graph))
        assert smp.N == 192 and smp.masked
        want = _sample(wu, cond, y0, cmask, lens)
        for b, L in enumerate(lens):
            assert same_bits(got[b, :L], want[b, :L]), (n, b, float((got[b, :L] - want[b, :L]).abs().max()))
            assert not got[b, L:].any()
    assert seen[0][0] is seen[1][0] and seen[0][1] is seen[1][1] and seen[0][1] is not None
    assert len(wu._samplers) == 2


# ------------------------------------------------------------------------------------------------ 10: codec and phoneme paths
def test_codec_paths_decode_every_row_alone(golden):
    """small_codec_text's model with tests/toy_codec.py: waves and last_sample_lens per row equal the row-alone decode, zero-filled;
    codes hold -1 in padding."""
    import voicebox_pytorch_amd as vbx
    from toy_codec import ToyCodec
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_codec_text")
    codec = ToyCodec(g["latent_dim"])
    vb = vbx.VoiceBox(dim=64, audio_enc_dec=codec, depth=2, dim_head=64, heads=2, time_hidden_dim=g["time_hidden_dim"],
                      ff_mult=g["ff_mult"], num_cond_tokens=50, dim_cond_emb=48, condition_on_text=True)
    vb.load_state_dict(g["state"], strict=False)
    w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev))
    ids, lens = g["ids"].to(dev), [40, 7, 23]
    assert ids.shape == (3, 40) and g["y0"].shape[:2] == (3, 40)
    kw = dict(cond=g["wave"].to(dev), semantic_token_ids=ids, steps=3, cond_scale=1.3, lens=lens)
    with rng_override(y0=g["y0"]):
        lat = w.sample(decode_to_audio=False, **kw)
    assert lat.shape == (3, 40, g["latent_dim"]) and w.last_sample_lens.tolist() == lens
    with rng_override(y0=g["y0"]):
        wave = w.sample(**kw)
    hop = codec.hop
    assert wave.shape == (3, 40 * hop) and w.last_sample_lens.tolist() == [L * hop for L in lens] and w.last_sample_lens.dtype == torch.int64
    with rng_override(y0=g["y0"]):
        codes = w.sample(decode_to_codes=True, **kw)
    assert codes.shape == (3, 40) and w.last_sample_lens.tolist() == lens
    for b, L in enumerate(lens):
        assert not lat[b, L:].any()
        assert same_bits(wave[b, :L * hop], codec.decode(lat[b:b + 1, :L].contiguous())[0]) and not wave[b, L * hop:].any()
        assert torch.equal(codes[b, :L], codec.decode_to_codes(lat[b:b + 1, :L])[0]) and (codes[b, L:] == -1).all()
    with rng_override(y0=g["y0"]):
        w.sample(cond=g["wave"].to(dev), semantic_token_ids=ids, steps=3, cond_scale=1.3)
    assert w.last_sample_lens is None


def test_lens_durations_regulates_on_the_device(golden):
    """lens="durations": a DurationPredictor of the duration golden, phoneme ids with -1 padding.  The kernel's aligned ids and
    lengths equal the CPU restatement; padding phonemes get no frames; the sample meets the leak test."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override
    from voicebox_pytorch_amd.sample_lens import durations_lens, length_regulate_restated

    c = golden("duration")["short_cond"]
    dp = vbx.DurationPredictor(num_phoneme_tokens=37, dim_phoneme_emb=32, dim=64, depth=2, dim_head=64, heads=2, **c["kw"])
    dp.load_state_dict(c["state"], strict=False)
    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=64, num_cond_tokens=37, depth=2, dim_head=64, heads=2, dim_cond_emb=48, condition_on_text=True)
    cfm = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, duration_predictor=dp).to(dev)
    ids = c["ids"].clone()
    K = ids.shape[1]
    ids[1, K - 3:], ids[2, K // 2:] = -1, -1  # padding phonemes on two rows
    # one cond for every call (the predictor's cond_mask draw depends on its frame count): longer than any aligned length
    ids, cond = ids.to(dev), torch.nn.functional.pad(c["cond"], (0, 0, 0, max(256 - c["cond"].shape[1], 0))).to(dev)
    draws = dict(coin=True, frac_lengths=torch.tensor([0.3, 0.6, 0.9]), rand=torch.tensor([0.1, 0.5, 0.8]))
    with rng_override(**draws):
        dur = cfm.duration_predictor.eval().forward_with_cond_scale(cond=cond, phoneme_ids=ids)
    aligned, lens = durations_lens(ids, dur)
    want_ids, want_lens = length_regulate_restated(ids.cpu(), dur.cpu())
    assert lens.dtype == torch.int32 and lens.tolist() == want_lens.tolist() and torch.equal(aligned.cpu(), want_ids)
    old = cfm.duration_predictor.align_phoneme_ids_with_durations(ids, dur)
    assert old.shape[1] > aligned.shape[1] or (old == -1).any()  # the path without lens samples the padding phonemes' frames
    # durations that exercise the clamp and the truncation, and more phonemes than one thread's worth
    Kb = 700
    gen = torch.Generator().manual_seed(3)
    big_ids = torch.randint(0, 37, (2, Kb), generator=gen)
    big_ids[0, 650:] = -1
    big_dur = torch.tensor([0.2, 1.0, 1.99, 7.5, -3.0]).repeat(2, Kb // 5)
    a2, l2 = durations_lens(big_ids.to(dev), big_dur.to(dev))
    w2, wl2 = length_regulate_restated(big_ids, big_dur)
    assert l2.tolist() == wl2.tolist() and torch.equal(a2.cpu(), w2)
    # the sample: shape, lengths, and nothing past a length reaches a real frame
    n, lens_l = aligned.shape[1], lens.tolist()
    gen = torch.Generator().manual_seed(1)
    y0 = torch.randn(3, n, 64, generator=gen)
    assert n <= cond.shape[1]
    cond_n = cond.cpu()  # sample() cuts it to the aligned length itself
    with rng_override(y0=y0, **draws):
        a = cfm.sample(cond=cond_n.to(dev), phoneme_ids=ids, steps=3, lens="durations")
    assert a.shape == (3, n, 64) and cfm.last_sample_lens.tolist() == lens_l
    safe = [max(L, K) for L in lens_l]  # the duration predictor reads the first K frames of cond: plant past them
    with rng_override(y0=plant(y0, lens_l, gen), **draws):
        b = cfm.sample(cond=plant(cond_n, safe, gen).to(dev), phoneme_ids=ids, steps=3, lens="durations")
    assert same_bits(a, b)
    for r, L in enumerate(lens_l):
        assert not a[r, L:].any() and a[r, :L].abs().sum() > 0
    with rng_override(y0=y0):  # the same frames from the aligned ids directly
        s = cfm.sample(cond=cond_n.to(dev), semantic_token_ids=aligned, steps=3, lens=lens)
    assert same_bits(s, a)


# ------------------------------------------------------------------------------------------------ 11: lens=None is the parent
def test_unmasked_sample_gives_the_parents_bits():
    """With lens=None sample() launches what it launched before lens existed: tests/golden/sample_lens_parent.json holds the SHA-256 of
    four outputs recorded on the parent commit (tests/golden/make_sample_lens_parent.py, whose cases() is replayed here).  The outputs
    pass through libm, so the hashes only mean something under the toolchain that produced them: where torch.version.hip or hipcc's
    `HIP version` line differ from the recorded ones the test skips and names both."""
    spec = importlib.util.spec_from_file_location("make_sample_lens_parent", os.path.join(HERE, "golden", "make_sample_lens_parent.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(os.path.join(HERE, "golden", "sample_lens_parent.json")) as fh:
        rec = json.load(fh)
    recorded, running = (rec["torch_version_hip"], rec["hipcc_version"]), maker.toolchain()
    if running != recorded:
        pytest.skip(f"hashes recorded under {recorded}, running under {running}")
    want, wrong = rec["sha256"], []
    for name, fn in maker.cases():
        got = fn()
        torch.cuda.synchronize()
        if maker.sha(got) != want[name]:
            wrong.append(name)
    assert len(want) == 4 and not wrong, wrong
