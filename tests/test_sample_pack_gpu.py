"""sample(lens=, pack=True) on the device: a ragged batch as one packed row stream (include/vbx.h "packed rows").  The two new
kernels against the existing ones on a segment alone, bit for bit, through the C ABI; the sampler against the yardstick of the lens=
tests (tests/test_sample_lens_cpu.py masked_sample, the small_wc golden's network, inputs seeded as in test_sample_lens_gpu.py).
Every line that starts with PARITY is a measured figure (profiles/sample_pack_parity.txt is those lines of one run)."""
import os

import pytest
import torch

from oracle import restate
from test_sample_lens_cpu import masked_sample, plant

pytestmark = pytest.mark.gpu
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
B, N, STEPS = 4, 200, 5
# R = 16 register rows lead every segment: R + len hits 63, 64, 65, 128, 129 and 216 -> segments of 128 and 256 rows, Mp = 640 and 768
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


def _reference(method, lens, n=N, b=B, seed=21):
    def build():
        g = _golden()
        cond, y0, cmask = _inputs(n, b, seed)
        return masked_sample(g["state"], restate.Cfg(**g["cfg"]), y0, cond, cmask, lens, STEPS, method=method, dtype=torch.float32)
    return cached(("ref", method, tuple(lens), n, b, seed), build)


def _sample(wrapper, cond, y0, cmask, lens, **kw):
    from voicebox_pytorch_amd.masks import rng_override

    with rng_override(y0=y0):
        return wrapper.sample(cond=cond.to(dev), cond_mask=cmask.to(dev), steps=STEPS, lens=lens, **kw)


def _row_errors(out, ref, lens):
    return [rel(out[b, :L], ref[b, :L]) for b, L in enumerate(lens)]


def _tables(klens, R=0, extra_tiles=1):
    """device tables of segments with these key lengths (seg_klen = klen), `extra_tiles` tiles of -1 at the end"""
    from voicebox_pytorch_amd import sample_pack as sp

    plan = sp.pack_plan([k - R for k in klens], R)
    Mp = plan.Mp + 128 * extra_tiles
    tile_seg = torch.cat((plan.tile_seg, torch.full((extra_tiles,), -1, dtype=torch.int32)))
    sp.check_tables(plan.seg_start, plan.seg_klen, tile_seg, Mp, len(klens))
    return plan, Mp, (plan.seg_start.to(dev), plan.seg_klen.to(dev), tile_seg.to(dev))


# ------------------------------------------------------------------------------------------------ 1: the attention kernel
@pytest.mark.parametrize("klens", [(1, 63, 64), (65, 128, 129), (216, 255, 256)])
def test_attn_fwd_segs_equals_attn_fwd_lens_on_the_segment_alone(klens):
    """vbx_attn_fwd_segs through the C ABI, H = 2, three segments and a -1 tile: for every segment the live query rows (fp16 and bf16
    output) and lse are bit-equal to vbx_attn_fwd_lens on that segment alone (B = 1, Np = its aligned size, key_lens = klen, mask
    NULL: the full-tile role).  Then NaN on every dead row of q, k and v, inside the segments and past the last one: the live outputs
    keep their bits, there is no NaN anywhere, the -1 tile holds zeros and lse 1e30.  Buffers are NaN-filled with a guard row."""
    from voicebox_pytorch_amd import _lib as L

    H, I = 2, 128
    plan, Mp, tabs = _tables(klens)
    gen = torch.Generator().manual_seed(sum(klens))
    q, k, v = ((torch.randn(1, H, Mp, 64, generator=gen) * s).half().to(dev) for s in (1.5, 1.0, 1.0))
    nans = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=dev)

    def run_segs(q, k, v):
        o16, ob, lse = nans((Mp + 1, I), torch.float16), nans((Mp + 1, I), torch.bfloat16), nans((H * Mp + 1,), torch.float32)
        L.call("vbx_attn_fwd_segs", q, k, v, *tabs, o16, ob, lse, H, Mp, 10.0, _st())
        torch.cuda.synchronize()
        assert o16[-1].isnan().all() and ob[-1].isnan().all() and lse[-1].isnan()  # nothing past the end
        return o16[:-1], ob[:-1], lse[:-1].view(H, Mp)

    def run_alone(s0, size, kl):
        cut = lambda t: t[:, :, s0:s0 + size].contiguous()
        o16, ob, lse = nans((size + 1, I), torch.float16), nans((size + 1, I), torch.bfloat16), nans((H * size + 1,), torch.float32)
        L.call("vbx_attn_fwd_lens", cut(q), cut(k), cut(v), None, torch.tensor([kl], dtype=torch.int32, device=dev), o16, ob, lse, 1, H, size,
               10.0, _st())
        torch.cuda.synchronize()
        return o16[:-1], ob[:-1], lse[:-1].view(H, size)

    got = run_segs(q, k, v)
    live = torch.zeros(Mp, dtype=torch.bool, device=dev)
    for s, kl in enumerate(klens):
        s0, size = int(plan.seg_start[s]), -(-kl // 128) * 128
        want = run_alone(s0, size, kl)
        live[s0:s0 + kl] = True
        assert same_bits(got[0][s0:s0 + kl], want[0][:kl]) and same_bits(got[1][s0:s0 + kl], want[1][:kl]), (klens, s)
        assert same_bits(got[2][:, s0:s0 + kl], want[2][:, :kl]), (klens, s)
        assert got[0][s0:s0 + kl].float().abs().sum() > 0
    dead = ~live
    bad = lambda t: torch.where(dead[None, None, :, None], torch.full_like(t, float("nan")), t)
    got2 = run_segs(bad(q), bad(k), bad(v))
    assert not any(t.isnan().any() for t in got2), klens
    assert same_bits(got2[0][live], got[0][live]) and same_bits(got2[1][live], got[1][live]) and same_bits(got2[2][:, live], got[2][:, live])
    last = plan.Mp  # the -1 tile
    for g in (got, got2):
        assert not g[0][last:].any() and not g[1][last:].float().any() and (g[2][:, last:] == 1e30).all()


# ------------------------------------------------------------------------------------------------ 2: the conv_embed kernel
@pytest.mark.parametrize("ksize", [31, 7])
@pytest.mark.parametrize("D", [64, 128])
def test_convpos_fwd_segs_equals_convpos_fwd_on_the_row_alone(D, ksize):
    """vbx_convpos_fwd_segs, R = 16, lengths (200, 47, 5, 1) and a -1 tile: frame rows bit-equal to vbx_convpos_fwd on the row alone
    (B = 1, N = len, no mask), register rows bit-equal to the register parameter, dead rows exactly 0; garbage (1e3 randn) in e on
    register and dead rows changes no bit."""
    from voicebox_pytorch_amd import _lib as L

    R, lens = 16, (200, 47, 5, 1)
    plan, Mp, tabs = _tables([R + v for v in lens], R=R)
    gen = torch.Generator().manual_seed(D + ksize)
    e = torch.randn(Mp, D, generator=gen).to(dev)
    w, bias, reg = (torch.randn(s, generator=gen).to(dev) for s in ((D, ksize), (D,), (R, D)))
    w = w * 0.3

    def run(e):
        xs = torch.full((Mp + 1, D), float("nan"), device=dev)
        L.call("vbx_convpos_fwd_segs", e, w, bias, reg, *tabs, xs, Mp, R, D, ksize, _st())
        torch.cuda.synchronize()
        assert xs[-1].isnan().all()
        return xs[:-1]

    got = run(e)
    frame = torch.zeros(Mp, dtype=torch.bool, device=dev)
    for b, v in enumerate(lens):
        s0 = int(plan.seg_start[b])
        size = -(-(R + v) // 128) * 128
        alone = torch.full((R + v + 1, D), float("nan"), device=dev)
        L.call("vbx_convpos_fwd", e[s0 + R:s0 + R + v].contiguous(), w, bias, None, reg, alone, 1, v, R, D, ksize, _st())
        torch.cuda.synchronize()
        assert alone[-1].isnan().all()
        assert same_bits(got[s0 + R:s0 + R + v], alone[R:R + v]), (b, v, float((got[s0 + R:s0 + R + v] - alone[R:R + v]).abs().max()))
        assert same_bits(got[s0:s0 + R], reg) and same_bits(alone[:R], reg)
        assert not got[s0 + R + v:s0 + size].any() and not got[s0 + R + v:s0 + size].isnan().any()
        frame[s0 + R:s0 + R + v] = True
    assert not got[plan.Mp:].any() and not got.isnan().any()
    garbage = torch.where(frame[:, None], e, 1e3 * torch.randn(Mp, D, generator=gen).to(dev))
    assert same_bits(run(garbage), got)


# ------------------------------------------------------------------------------------------------ 3: against the restatement
@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("method", ["midpoint", "euler", "rk4"])
def test_packed_sample_matches_the_restatement(method, use_graph, li):
    """Real frames of every row within 2e-3 relative L2 of the fp32 restatement loop (the bound the project holds this network and
    these inputs to; the masked path measures 3 - 6e-4) and padding exactly 0: all fixed-grid methods, eager and captured."""
    lens = LENS[li]
    cond, y0, cmask = _inputs()
    w = _wrapper(method)
    out = _sample(w, cond, y0, cmask, list(lens), use_graph=use_graph, pack=True)
    smp = next(iter(w._samplers.values()))
    assert smp.packed and not smp.masked and smp.split == 1 and smp.B == 1 and smp.N == (640, 768)[li]
    assert out.shape == (B, N, cond.shape[-1]) and out.is_contiguous()
    assert w.last_sample_lens.dtype == torch.int64 and w.last_sample_lens.tolist() == list(lens)
    errs = _row_errors(out, _reference(method, lens), lens)
    print(f"PARITY packed vs restatement {method} {'graph' if use_graph else 'eager'} lens {lens}: rel L2 per row",
          " ".join(f"{e:.2e}" for e in errs))
    for b, L in enumerate(lens):
        assert torch.equal(out[b, L:], torch.zeros_like(out[b, L:])), (b, L)
    assert max(errs) < 2e-3, errs
    if use_graph:  # a second call replays the captured graph on fresh inputs
        assert smp.graph is not None
        assert same_bits(_sample(w, cond, y0, cmask, list(lens), use_graph=True, pack=True), out)
        assert next(iter(w._samplers.values())) is smp


# ------------------------------------------------------------------------------------------------ 4: nothing leaks
@pytest.mark.parametrize("method", ["midpoint", "rk4"])
def test_padding_cannot_leak_into_a_packed_sample(method):
    """The same call twice, the second with garbage past the lengths in cond, cond_mask and the y0 override: the whole result is
    bit-equal."""
    lens = LENS[0]
    cond, y0, cmask = _inputs()
    gen = torch.Generator().manual_seed(77)
    w = _wrapper(method)
    a = _sample(w, cond, y0, cmask, list(lens), pack=True)
    b = _sample(w, plant(cond, lens, gen), plant(y0, lens, gen), plant(cmask, lens, gen), torch.tensor(lens, device=dev), pack=True)
    assert len(w._samplers) == 1
    assert same_bits(a, b), float((a - b).abs().max())
    for r, L in enumerate(lens):
        assert not a[r, L:].any() and a[r, :L].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 5: the row alone
def _alone_tolerances(cond, y0, cmask, lens, masked_out, ref):
    """per row: (the row by itself at N = len_b on today's path, max(2 x the distance between two such runs that differ only in batch
    position, the masked path's distance to the restatement)) -- the construction of test_masked_row_equals_the_row_alone; no figure
    comes from the packed path"""
    from voicebox_pytorch_amd.masks import rng_override

    nb = cond.shape[0]
    to_ref = _row_errors(masked_out, ref, lens)
    res = []
    for b, L in enumerate(lens):
        c1, y1, m1 = cond[b:b + 1, :L], y0[b:b + 1, :L], cmask[b:b + 1, :L]
        o = (b + 1) % nb  # a filler row in front, cut to the same length
        c2, y2, m2 = torch.cat([cond[o:o + 1, :L], c1]), torch.cat([y0[o:o + 1, :L], y1]), torch.cat([cmask[o:o + 1, :L], m1])
        plain = _wrapper()
        with rng_override(y0=y1):
            alone = plain.sample(cond=c1.to(dev), cond_mask=m1.to(dev), steps=STEPS)
        with rng_override(y0=y2):
            second = plain.sample(cond=c2.to(dev), cond_mask=m2.to(dev), steps=STEPS)[1:]
        position = rel(second, alone)
        res.append((alone, max(2 * position, to_ref[b]), position, to_ref[b]))
    return res


def _wc_case(n, b, seed, lens):
    """inputs, the masked path's result and the per-row tolerances of one (B, N) case, computed once"""
    def build():
        cond, y0, cmask = _inputs(n, b, seed)
        masked = _sample(_wrapper(), cond, y0, cmask, list(lens))
        return cond, y0, cmask, masked, _alone_tolerances(cond, y0, cmask, lens, masked, _reference("midpoint", lens, n, b, seed))
    return cached(("case", n, b, seed, tuple(lens)), build)


def test_packed_row_equals_the_row_alone():
    """Row b of a packed B = 4 midpoint call on its real frames against sample() of that row by itself at N = len_b (today's path),
    at the tolerance of test_sample_lens_gpu.test_masked_row_equals_the_row_alone.  Printed, not asserted: whether packed and masked
    agree bit for bit."""
    lens = LENS[0]
    cond, y0, cmask, masked, tols = _wc_case(N, B, 21, lens)
    out = _sample(_wrapper(), cond, y0, cmask, list(lens), pack=True)
    for b, L in enumerate(lens):
        alone, tol, position, to_ref = tols[b]
        d = rel(out[b:b + 1, :L], alone)
        print(f"PARITY packed row alone: row {b} len {L}: packed-in-batch vs alone {d:.2e}; alone at batch position 0 vs 1 {position:.2e}; "
              f"masked-in-batch vs restatement {to_ref:.2e}; tolerance {tol:.2e}; packed == masked bit for bit: "
              f"{same_bits(out[b, :L], masked[b, :L])} (rel {rel(out[b, :L], masked[b, :L]):.2e})")
        assert d <= tol, (b, L, d, tol)


# ------------------------------------------------------------------------------------------------ 6: one sampler per bucket
def test_pack_bucket_shares_one_sampler():
    """(B, N) = (4, 200) and (3, 130) at pack_bucket 1024: one _samplers entry, the same sampler object and the same graph object;
    real frames within the row-alone tolerance of the same calls without a bucket, padding 0."""
    w, wu = _wrapper(), _wrapper()
    seen = []
    for n, b, seed, lens in ((N, B, 21, LENS[0]), (130, 3, 130, (130, 100, 47))):
        cond, y0, cmask, _, tols = _wc_case(n, b, seed, lens)
        got = _sample(w, cond, y0, cmask, list(lens), pack=True, pack_bucket=1024)
        assert got.shape == (b, n, cond.shape[-1]) and len(w._samplers) == 1
        smp = next(iter(w._samplers.values()))
        seen.append((smp, smp.graph))
        assert smp.N == 1024 and smp.packed and w.last_sample_stats["packed_rows"] == 1024
        want = _sample(wu, cond, y0, cmask, list(lens), pack=True)
        assert wu.last_sample_stats["packed_rows"] == (640, 512)[len(seen) - 1]
        for r, L in enumerate(lens):
            d = rel(got[r, :L], want[r, :L])
            print(f"PARITY pack_bucket 1024 vs exact packing: B {b} N {n} row {r} len {L}: rel {d:.2e} (bit-equal: "
                  f"{same_bits(got[r, :L], want[r, :L])}); tolerance {tols[r][1]:.2e}")
            assert d <= tols[r][1], (n, r, d, tols[r][1])
            assert not got[r, L:].any()
    assert seen[0][0] is seen[1][0] and seen[0][1] is seen[1][1] and seen[0][1] is not None


# ------------------------------------------------------------------------------------------------ 7: guidance and text
def test_packed_guidance_and_text(golden):
    """small_text's network, cond_scale 1.3, one id per frame: the packed call against masked_sample(cond_token_ids=) at the bound
    the masked path meets on the same inputs (measured here and printed), or 2e-3 where that is larger."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_text")
    vb = vbx.VoiceBox(dim=64, num_cond_tokens=50, dim_cond_emb=48, depth=2, dim_head=64, heads=2, condition_on_text=True)
    vb.load_state_dict(g["state"], strict=False)
    w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev).eval())
    cfg = restate.Cfg(dim=64, depth=2, heads=2, dim_head=64)
    lens = (40, 17, 23)
    cmask = torch.rand(3, 40, generator=torch.Generator().manual_seed(5)) < 0.6
    ref = masked_sample(g["state"], cfg, g["y0"], g["cond"], cmask, lens, 3, dtype=torch.float32, cond_token_ids=g["ids_n"], cond_scale=1.3)
    res = {}
    for pack in (False, True):
        with rng_override(y0=g["y0"]):
            out = w.sample(cond=g["cond"].to(dev), cond_mask=cmask.to(dev), semantic_token_ids=g["ids_n"].to(dev), steps=3, cond_scale=1.3,
                           lens=list(lens), **(dict(pack=True) if pack else {}))
        res[pack] = _row_errors(out, ref, lens)
        assert out.shape == (3, 40, 64) and all(not out[b, L:].any() for b, L in enumerate(lens))
        assert w.last_sample_stats["nfe"] == 2 * 2 * 2  # two intervals, two stages, two forwards each
    print("PARITY guided text vs restatement: masked", " ".join(f"{e:.2e}" for e in res[False]), "packed", " ".join(f"{e:.2e}" for e in res[True]))
    assert max(res[True]) <= max(max(res[False]), 2e-3), res


# ------------------------------------------------------------------------------------------------ 8: the codec path
def test_packed_codec_paths_decode_every_row_alone(golden):
    """small_codec's model (latent 100 into dim 64) with tests/toy_codec.py: latents, waves and codes with last_sample_lens, -1
    codes and the per-row decode, as test_sample_lens_gpu.test_codec_paths_decode_every_row_alone states them for lens=."""
    import voicebox_pytorch_amd as vbx
    from toy_codec import ToyCodec
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_codec")
    codec = ToyCodec(g["latent_dim"])
    vb = vbx.VoiceBox(dim=64, audio_enc_dec=codec, depth=2, dim_head=64, heads=2, time_hidden_dim=g["time_hidden_dim"],
                      ff_mult=g["ff_mult"], num_cond_tokens=500, condition_on_text=False)
    vb.load_state_dict(g["state"], strict=False)
    w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev))
    lens = [40, 7]
    kw = dict(cond=g["wave_cond"].to(dev), steps=5, lens=lens, pack=True)
    with rng_override(y0=g["y0"]):
        lat = w.sample(decode_to_audio=False, **kw)
    assert lat.shape == (2, 40, g["latent_dim"]) and w.last_sample_lens.tolist() == lens
    with rng_override(y0=g["y0"]):
        masked = w.sample(cond=g["wave_cond"].to(dev), steps=5, lens=lens, decode_to_audio=False)
    print("PARITY codec latents packed vs masked: rel per row", " ".join(f"{rel(lat[b, :L], masked[b, :L]):.2e}" for b, L in enumerate(lens)))
    assert rel(lat[0], g["sample5"][0]) < 0.02  # the full row: the reference's own sample (test_codec_model_vs_reference's bound)
    with rng_override(y0=g["y0"]):
        wave = w.sample(**kw)
    hop = codec.hop
    assert wave.shape == (2, 40 * hop) and w.last_sample_lens.tolist() == [L * hop for L in lens] and w.last_sample_lens.dtype == torch.int64
    with rng_override(y0=g["y0"]):
        codes = w.sample(decode_to_codes=True, **kw)
    assert codes.shape == (2, 40) and w.last_sample_lens.tolist() == lens
    for b, L in enumerate(lens):
        assert not lat[b, L:].any()
        assert same_bits(wave[b, :L * hop], codec.decode(lat[b:b + 1, :L].contiguous())[0]) and not wave[b, L * hop:].any()
        assert torch.equal(codes[b, :L], codec.decode_to_codes(lat[b:b + 1, :L])[0]) and (codes[b, L:] == -1).all()


# ------------------------------------------------------------------------------------------------ 9: stats
def test_packed_stats_are_the_plans():
    from voicebox_pytorch_amd import sample_pack as sp

    cond, y0, cmask = _inputs()
    w = _wrapper()
    for li, bucket in ((0, None), (1, None), (1, 1024)):
        _sample(w, cond, y0, cmask, list(LENS[li]), pack=True, pack_bucket=bucket)
        plan = sp.pack_plan(LENS[li], 16, bucket, N=N)
        s = w.last_sample_stats
        assert (s["packed_rows"], s["live_rows"], s["padded_rows"]) == (plan.Mp, plan.live_rows, plan.padded_rows) and plan.padded_rows == B * (16 + N)
        assert s["method"] == "midpoint" and s["nfe"] == 2 * (STEPS - 1)
    _sample(w, cond, y0, cmask, list(LENS[0]))  # the masked path's stats are what they were
    assert "packed_rows" not in w.last_sample_stats
