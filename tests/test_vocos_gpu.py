"""VocosDecoder on the device (csrc/vocos.hip, the GELU epilogue of csrc/gemm.hip, vbx_istft of csrc/griffinlim.hip) against the fp64
restatement tests/vocos_ref.py, kernel by kernel and whole.  Parity with the `vocos` library is UNPINNED (the library is absent).

Whole-decoder error = max |difference| / RMS of the wave.  Figures measured on an MI355X over seeds 0, 1, 2 (`pytest -s` prints
them; profiles/vocos_parity.txt keeps them):
  (a) against the emulated-precision restatement (fp16 at the device's rounding points): 1.9e-4 .. 4.4e-3; BOUND_A = 2 x the
      largest of the three seeds and three shapes.  Nothing but the order of the fp32 sums differs, and that is what the spread
      is: a value that the two orders leave on different sides of an fp16 rounding boundary moves by a whole fp16 ulp, and one such
      flip in the 64-wide LayerNorm output in front of the head shifts every phase of its frame by ~1e-3 rad.  (On the CPU, noise
      of 2e-7 relative in front of each rounding of the restatement moves its own wave by 1.4e-3 .. 4.3e-3.)  The margin of 2 is
      for the seed-to-seed spread of those flips;
  (b) against the unrounded fp64 restatement: 5.4e-3 .. 7.0e-3; BOUND_B = 2 x the largest, a sanity bound (it measures what fp16
      operands cost).
test_bound_is_far_below_every_fault (CPU, fp64 only) holds BOUND_A against what a wrong decoder would move."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import vocos_ref as vr
from attn_check import rel_err

gpu = pytest.mark.gpu
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))

SMALL = dict(input_channels=8, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64)
REAL = dict(input_channels=100, dim=512, intermediate_dim=1536, num_layers=2, n_fft=1024, hop_length=256)
WHOLE = [("small-9", SMALL, 2, 9), ("small-40", SMALL, 2, 40), ("real-12", REAL, 1, 12)]
SEEDS = (0, 1, 2)
BOUND_A = 2 * 4.359e-3  # largest of 9 (3 shapes x 3 seeds): small-40, seed 0
BOUND_B = 2 * 7.020e-3  # sanity bound; largest of 9: small-40, seed 2
HEAD_BOUND = 2 * 6.969e-8  # 2 x the largest measured distance (the magnitude's); see test_head_magnitude_and_phasor


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------- pack
@gpu
@pytest.mark.parametrize("C", [8, 100])
@pytest.mark.parametrize("frames", [1, 5, 9])
def test_pack_input(L, C, frames):
    """bit for bit the fp16 rounding of the restated im2col: fewer frames than taps (both paddings overlap), pad columns, a second
    batch element of another constant (a halo read across the batch boundary would show), nothing past the last row"""
    g = torch.Generator().manual_seed(C + frames)
    x = torch.randn(2, C, frames, generator=g)
    x[1] = 3.25
    Kp = L.lib().vbx_vocos_kp(C)
    assert Kp % 32 == 0 and 7 * C <= Kp < 7 * C + 32
    out = torch.full((2 * frames + 1, Kp), float("nan"), dtype=torch.float16, device=dev)
    L.call("vbx_vocos_pack_input", x.to(dev), out, 2, C, frames, 0, st())
    exp = vr.im2col(x.double(), Kp).half()
    assert torch.equal(bits(out[:-1].cpu()), bits(exp))
    assert bool(torch.isnan(out[-1]).all())
    if 7 * C < Kp:
        assert float(out[:-1, 7 * C:].float().abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("C,frames", [(8, 5), (100, 9)])
def test_pack_input_log(L, C, frames):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2, C, frames, generator=g).abs() * 3.0
    x[0, 0, 0], x[0, 1, 1], x[1, 2, 2], x[1, 0, -1] = 0.0, -2.0, 1e-9, 1.0
    x[0, -1] = -x[0, -1]
    Kp = L.lib().vbx_vocos_kp(C)
    out = torch.full((2 * frames + 1, Kp), float("nan"), dtype=torch.float16, device=dev)
    L.call("vbx_vocos_pack_input", x.to(dev), out, 2, C, frames, 1, st())
    exp = vr.im2col(torch.log(torch.clamp(x, min=1e-7)), Kp).half().float()  # fp32 log, zero padding AFTER the log
    got = out[:-1].float().cpu()
    ulp = torch.maximum(exp.abs() * 2.0 ** -10, torch.tensor(2.0 ** -24))
    assert bool(((got - exp).abs() <= ulp).all()) and bool(torch.isnan(out[-1]).all())
    assert bool((got[exp == 0.0] == 0.0).all()) and float(exp.min()) < -16.0  # log(1e-7): the floor was reached


# ----------------------------------------------------------------------------- depthwise convolution + LayerNorm
@gpu
@pytest.mark.parametrize("D", [64, 512])
@pytest.mark.parametrize("frames", [1, 3, 9, 130])
def test_dwconv_layernorm(L, D, frames):
    g = torch.Generator().manual_seed(D + frames)
    x = torch.randn(2, frames, D, generator=g)
    x[1] += 2.0
    w, cb = torch.randn(D, 1, 7, generator=g) * 7 ** -0.5, 0.3 * torch.randn(D, generator=g)
    lw, lb = 1.0 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    taps = w[:, 0, :].t().contiguous()
    y = torch.full((2 * frames + 1, D), float("nan"), dtype=torch.float16, device=dev)
    L.call("vbx_vocos_dwconv_ln", x.to(dev), taps.to(dev), cb.to(dev), lw.to(dev), lb.to(dev), y, 2, frames, D, 1e-6, st())
    conv = F.conv1d(x.double().transpose(1, 2), w.double(), cb.double(), padding=3, groups=D).transpose(1, 2)
    ref = F.layer_norm(conv, (D,), lw.double(), lb.double(), 1e-6).reshape(2 * frames, D)
    err = rel_err(y[:-1], ref)
    print(f"dwconv_ln D {D} frames {frames}: rel_err {err:.3e}")
    assert err < 6e-4 and bool(torch.isnan(y[-1]).all())
    y2 = torch.full((2 * frames + 1, D), float("nan"), dtype=torch.float16, device=dev)
    L.call("vbx_vocos_dwconv_ln", x.to(dev), None, None, lw.to(dev), lb.to(dev), y2, 2, frames, D, 1e-6, st())
    ref2 = F.layer_norm(x.double(), (D,), lw.double(), lb.double(), 1e-6).reshape(2 * frames, D)
    assert rel_err(y2[:-1], ref2) < 6e-4 and bool(torch.isnan(y2[-1]).all())


# ----------------------------------------------------------------------------- GELU epilogue and routing
def gemm_desc(L, mode, epi, M, N, K, ldc, f16=0, ptrs=()):
    """a descriptor with placeholder buffers (vbx_gemm_route tests pointers for null and alignment only)"""
    d = L.GemmDesc()
    d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16 = mode, epi, M, N, K, K, K, ldc, f16
    for name in ("A", "B", "C") + tuple(ptrs):
        setattr(d, name, 4096)
    return d


NT_SHAPES = [(300, 264, 200), (128, 128, 64), (8320, 512, 1024), (77, 1536, 512), (8320, 512, 1000), (8200, 512, 64), (4160, 512, 1408),
             (8320, 1024, 1024), (8320, 1024, 512), (1234, 1408, 512), (70, 576, 512)]
GEGLU_SHAPES = [(341, 384), (405, 448)]
ROUTE_SELECTS = (0, 1, 2, 3, 4)


def route_cases(L):
    """the descriptors tests/test_ops_gpu.py::test_gemm_nt_bf16_f32 and ::test_gemm_geglu_epilogue hand to vbx_gemm"""
    for M, N, K in NT_SHAPES:
        yield f"nt {M}x{N}x{K} bf16+bias", gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_BF16, M, N, K, N, ptrs=("bias",))
        yield f"nt {M}x{N}x{K} f32+bias+resid+copy", gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_F32, M, N, K, N, ptrs=("bias", "resid", "C2"))
        yield f"nt {M}x{N}x{K} f32", gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_F32, M, N, K, N)
        yield f"nt {M}x{N}x{K} bf16", gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_BF16, M, N, K, N)
    for Fd, Fp in GEGLU_SHAPES:
        yield f"geglu {Fp} bf16 train", gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_GEGLU, 200, 2 * Fp, 128, Fp, ptrs=("bias", "C2"))
        yield f"geglu {Fp} f16 train", gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_GEGLU, 200, 2 * Fp, 128, Fp, f16=1, ptrs=("bias", "C2", "C3"))


def routes_now(L, lib):
    out = {}
    try:
        for sel in ROUTE_SELECTS:
            lib.vbx_gemm_select(sel)
            for key, d in route_cases(L):
                out.setdefault(key, []).append(lib.vbx_gemm_route(d))
    finally:
        lib.vbx_gemm_select(0)
    return out


@gpu
def test_existing_descriptors_route_as_before(L):
    """tests/golden/gemm_routes_parent.json: vbx_gemm_route of these descriptors under vbx_gemm_select 0 .. 4, recorded on the commit
    before VBX_EPI_GELU existed"""
    with open(os.path.join(HERE, "golden", "gemm_routes_parent.json")) as fh:
        rec = json.load(fh)
    assert rec["selects"] == list(ROUTE_SELECTS)
    assert routes_now(L, L.lib()) == rec["routes"]


GELU_SHAPES = [(200, 1536, 512), (77, 192, 64), (300, 264, 200)]


@gpu
@pytest.mark.parametrize("M,N,K", GELU_SHAPES)
@pytest.mark.parametrize("select", [0, 1])
def test_gemm_gelu_epilogue(L, M, N, K, select):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).half()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    bias = torch.randn(N, generator=g)
    out = torch.full((M + 1, N), float("nan"), dtype=torch.float16, device=dev)
    Ad, Wd, bd = A.to(dev), W.to(dev), bias.to(dev)
    d = gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_GELU, M, N, K, N, f16=1)
    d.A, d.B, d.C, d.bias = Ad.data_ptr(), Wd.data_ptr(), out.data_ptr(), bd.data_ptr()
    L.lib().vbx_gemm_select(select)
    try:
        assert L.lib().vbx_gemm(d, st()) == 0, L.lib().vbx_last_error()
    finally:
        L.lib().vbx_gemm_select(0)
    ref = F.gelu(A.double() @ W.double().t() + bias.double())
    err = rel_err(out[:M], ref)
    print(f"gelu epilogue {M}x{N}x{K} select {select}: rel_err {err:.3e}")
    assert err < 6e-4 and bool(torch.isnan(out[M]).all())


@gpu
def test_gelu_routes_to_the_128_wide_tiles(L):
    try:
        for sel in ROUTE_SELECTS:
            L.lib().vbx_gemm_select(sel)
            for M, N, K in GELU_SHAPES + [(8200, 1536, 512), (301, 1536, 512)]:
                d = gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_GELU, M, N, K, N, f16=1, ptrs=("bias",))
                assert L.lib().vbx_gemm_route(d) in (64, 128, 160), (sel, M, N, K)
    finally:
        L.lib().vbx_gemm_select(0)
    d = gemm_desc(L, L.VBX_GEMM_NT, L.VBX_EPI_GELU, 64, 64, 64, 64, f16=0, ptrs=("bias",))
    assert L.lib().vbx_gemm_route(d) < 0  # fp16 operands only


# ----------------------------------------------------------------------------- head
@gpu
def test_head_magnitude_and_phasor(L):
    """m over [-12, 6] (both sides of log 100), p over [-40, 40] (far outside the fast intrinsics' range), against fp64 of the same
    fp32 inputs, relative for the magnitude and absolute for cos / sin.  HIP's math accuracy tables (2 ulp for expf / sinf / cosf,
    which would give 4 x 2^-23) are not part of the documents a ROCm installation carries, so the bound is measured instead: magnitude
    7.0e-8, cos 5.6e-8, sin 5.7e-8 on an MI355X (profiles/vocos_parity.txt), x 2.  The fast intrinsics miss it by orders of
    magnitude at |p| ~ 40."""
    rows, nb, ld = 37, 129, 264
    g = torch.Generator().manual_seed(0)
    h = torch.full((rows, ld), float("nan"))
    h[:, :nb] = torch.linspace(-12.0, 6.0, rows * nb)[torch.randperm(rows * nb, generator=g)].reshape(rows, nb)
    h[:, nb:2 * nb] = (torch.rand(rows, nb, generator=g) * 2.0 - 1.0) * 40.0
    mag = torch.full((rows + 1, nb), float("nan"), device=dev)
    ph = torch.full((rows + 1, nb, 2), float("nan"), device=dev)
    L.call("vbx_vocos_head", h.to(dev), mag, ph, rows, nb, ld, st())
    m, p = h[:, :nb].double(), h[:, nb:2 * nb].double()
    ref = torch.clamp(torch.exp(m), max=100.0)
    assert int((m > math.log(100.0)).sum()) > 100 and int((m < math.log(100.0)).sum()) > 100
    e_mag = float(((mag[:rows].double().cpu() - ref) / ref).abs().max())
    e_cos = float((ph[:rows, :, 0].double().cpu() - torch.cos(p)).abs().max())
    e_sin = float((ph[:rows, :, 1].double().cpu() - torch.sin(p)).abs().max())
    print(f"head: mag rel {e_mag:.3e} cos abs {e_cos:.3e} sin abs {e_sin:.3e} (bound {HEAD_BOUND:.3e})")
    assert max(e_mag, e_cos, e_sin) < HEAD_BOUND
    assert bool((mag[:rows][(m > math.log(100.0)).to(dev)] == 100.0).all())
    assert bool(torch.isnan(mag[rows]).all()) and bool(torch.isnan(ph[rows]).all())


# ----------------------------------------------------------------------------- whole decoder
def whole_inputs(cfg, B, frames, seed):
    sd = vr.random_state(cfg["input_channels"], cfg["dim"], cfg["intermediate_dim"], cfg["num_layers"], cfg["n_fft"], seed)
    x = torch.randn(B, cfg["input_channels"], frames, generator=torch.Generator().manual_seed(1000 + seed))
    return sd, x


_refs = {}


def whole_refs(name, cfg, B, frames, seed):
    """(emulated-precision wave, fp64 wave, fraction of bins with m above log 100), computed once"""
    key = (name, seed)
    if key not in _refs:
        sd, x = whole_inputs(cfg, B, frames, seed)
        kw = dict(n_fft=cfg["n_fft"], hop=cfg["hop_length"])
        exact, m = vr.decode(sd, x, parts=True, **kw)
        _refs[key] = (vr.decode(sd, x, emulate=True, **kw), exact, float((m > math.log(100.0)).float().mean()))
    return _refs[key]


def build(cfg, sd):
    import voicebox_pytorch_amd as vbx

    m = vbx.VocosDecoder(**cfg)
    m.load_state_dict(sd)
    return m.to(dev).eval()


@gpu
@pytest.mark.parametrize("name,cfg,B,frames", WHOLE, ids=[w[0] for w in WHOLE])
def test_whole_decoder(name, cfg, B, frames):
    worst_a = worst_b = 0.0
    for seed in SEEDS:
        sd, x = whole_inputs(cfg, B, frames, seed)
        emu, exact, frac = whole_refs(name, cfg, B, frames, seed)
        assert 0.0 < frac <= 0.05, frac  # the clip at 100 is live, on a few bins
        wave = build(cfg, sd)(x.to(dev))
        assert wave.shape == (B, (frames - 1) * cfg["hop_length"]) and wave.dtype == torch.float32
        ea, eb = vr.wave_err(wave, emu), vr.wave_err(wave, exact)
        print(f"whole decoder {name} seed {seed}: (a) vs emulated precision {ea:.3e}  (b) vs fp64 {eb:.3e}  clipped bins {frac:.4f}")
        worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
    assert worst_a < BOUND_A, (worst_a, BOUND_A)
    assert worst_b < BOUND_B, ("sanity bound", worst_b, BOUND_B)


def test_bound_is_far_below_every_fault():
    """On the CPU, with the fp64 restatement alone: BOUND_A is at most a tenth of what each fault moves the wave by -- a dropped
    ConvNeXt block, a zeroed gamma, eps 1e-5 for 1e-6 (on inputs scaled by 0.01, embedding bias included, so that the first
    LayerNorm sees a variance of ~1e-4), no clip at 100."""
    for name, cfg, B, frames in WHOLE:
        sd, x = whole_inputs(cfg, B, frames, 0)
        kw = dict(n_fft=cfg["n_fft"], hop=cfg["hop_length"])
        exact = whole_refs(name, cfg, B, frames, 0)[1]
        for fault in [("drop_block", 0), ("drop_block", 1), ("zero_gamma", 1), ("no_clip",)]:
            moved = vr.wave_err(vr.decode(sd, x, fault=fault, **kw), exact)
            assert BOUND_A <= 0.1 * moved, (name, fault, moved)
        sd_s = dict(sd)
        sd_s["backbone.embed.bias"] = sd["backbone.embed.bias"] * 0.01
        emb = F.conv1d(0.01 * x.double(), sd_s["backbone.embed.weight"].double(), sd_s["backbone.embed.bias"].double(), padding=3)
        var = float(emb.var(dim=1, unbiased=False).mean())
        assert 3e-5 < var < 3e-4, var
        moved = vr.wave_err(vr.decode(sd_s, 0.01 * x, fault=("eps", 1e-5), **kw), vr.decode(sd_s, 0.01 * x, **kw))
        assert BOUND_A <= 0.1 * moved, (name, "eps", moved)


@gpu
def test_decode_reruns_and_repacks():
    sd, x = whole_inputs(SMALL, 2, 9, 0)
    m = build(SMALL, sd)
    xd = x.to(dev)
    a, b = m.decode(xd), m(xd)
    assert a.shape == (2, 8 * 64) and torch.equal(a, b)
    with torch.no_grad():
        m.backbone.convnext[1].pwconv2.weight.mul_(1.5)  # in place: the version counter moves, the next call packs again
    c = m(xd)
    sd2 = dict(sd)
    sd2["backbone.convnext.1.pwconv2.weight"] = sd["backbone.convnext.1.pwconv2.weight"] * 1.5
    assert not torch.equal(a, c) and vr.wave_err(c, vr.decode(sd2, x, emulate=True, n_fft=256, hop=64)) < BOUND_A
    assert vr.wave_err(a, vr.decode(sd2, x, emulate=True, n_fft=256, hop=64)) > 10 * BOUND_A


@gpu
def test_input_log_whole():
    sd, x = whole_inputs(SMALL, 2, 9, 1)
    x = x.abs() + 0.05
    m = build(dict(SMALL, input_log=True), sd)
    assert vr.wave_err(m(x.to(dev)), vr.decode(sd, x, input_log=True, emulate=True, n_fft=256, hop=64)) < BOUND_A


@gpu
def test_two_frames():
    """the shortest decode: vbx_istft does not ask for the analysis step's (frames - 1) * hop > n_fft / 2"""
    sd, x = whole_inputs(SMALL, 2, 2, 2)
    w = build(SMALL, sd)(x.to(dev))
    assert w.shape == (2, 64) and vr.wave_err(w, vr.decode(sd, x, emulate=True, n_fft=256, hop=64)) < BOUND_A


# ----------------------------------------------------------------------------- through the codec
@gpu
def test_through_logmelcodec():
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(0)
    voc = vbx.VocosDecoder(**dict(SMALL, input_channels=100))
    codec = vbx.LogMelCodec(vocoder=voc).to(dev)
    lat = (10.0 * torch.randn(2, 9, 100)).to(dev)
    a = codec.decode(lat)
    b = voc(torch.pow(10.0, 0.05 * lat.transpose(-1, -2)))
    assert a.shape == (2, 8 * 64) and torch.equal(a, b) and torch.isfinite(a).all()


@gpu
def test_voicebox_samples_a_wave_through_vocos():
    import mel_ref
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(0)
    codec = vbx.LogMelCodec(vocoder=vbx.VocosDecoder(**dict(SMALL, input_channels=100)))
    vb = vbx.VoiceBox(dim=64, depth=2, heads=2, audio_enc_dec=codec, condition_on_text=False).to(dev)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    wave = mel_ref.test_signal().to(dev)
    frames = 1 + wave.shape[1] // codec.hop_length
    w = wrapper.sample(cond=wave, steps=2)
    assert w.shape == (wave.shape[0], (frames - 1) * 64) and w.dtype == torch.float32 and torch.isfinite(w).all()
