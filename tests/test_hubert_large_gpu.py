"""voicebox_pytorch_amd.HubertLargeWithKmeans on the device (csrc/hubert.hip, "the large form") against the restatement
tests/hubert_large_ref.py, which tests/test_hubert_large_cpu.py pins to transformers.HubertModel.

Single kernels: fp64 on the same operands under DERIVED per-element bounds of the family's form (tests/test_hubert_gpu.py): with
ds the bound of a pre-norm value (any fp32 order of its K products) the LayerNorm over C channels adds _ln_bound below, then the GELU
epilogue |gelu'| <= 1.13 times that plus 8 * 2^-24 (|z| + |y|), then one fp16 rounding 2^-11 |y| + 2^-25.
Whole network: max |delta| / RMS against fp64 and against the emulated restatement, inside the tolerance MEASURED by
hubert_large_ref.tolerance_small(layer) -- a tenth of the smallest planted fault's movement, once for the un-normalised branch
(layer 2 of 4) and once for the final norm (layer 4 of 4); profiles/hubert_large_parity.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

import hubert_large_ref as LR
import hubert_ref as R
from test_hubert_gpu import _contract_ok, _draws, _gelu_bound, _wrapper

gpu = pytest.mark.gpu
dev = "cuda"
U24, U11 = 2.0 ** -24, 2.0 ** -11


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ln_bound(v, dv, gam, bet, eps):
    """v fp64 [.., C] the exact pre-norm values, dv >= |computed - exact| per element.  Two-pass fp32 LayerNorm over C as the kernels
    run it (a lane sums 8 values, a 6-level tree, a multiplication by 1 / C: c = 24 covers the 16 roundings of a sum and those of the
    deviations): the mean inherits max dv and carries c ulps of max |v|; var moves relatively by 2 max dv / std, so rstd by
    max dv * rstd relatively, plus c ulps; the affine adds two roundings.
    -> (z, dz): dz = rstd |gamma| (dv + max dv) + |z - beta| max dv rstd + 2^-24 [c rstd |gamma| max |v| + c |z - beta| + 4 (|z| + |beta|)]"""
    c = 24
    mean, var = v.mean(-1, keepdim=True), v.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    g, b = gam.double(), bet.double()
    z = (v - mean) * rstd * g + b
    dvm = dv.amax(-1, keepdim=True)
    dz = rstd * g.abs() * (dv + dvm) + (z - b).abs() * dvm * rstd + U24 * (c * rstd * g.abs() * v.abs().amax(-1, keepdim=True) + c * (z - b).abs() + 4 * (z.abs() + b.abs()))
    return z, dz


# ------------------------------------------------------------------------------------ conv0 + bias + LayerNorm + GELU
@gpu
@pytest.mark.parametrize("bias_on", [True, False])
@pytest.mark.parametrize("C", [32, 512])
def test_conv0_layernorm(C, bias_on):
    """Rows with a DC offset of 100.  dv = (k0 + 1) 2^-24 sum |w x| for the fmaf chain, + 2^-24 |v| for the bias; then _ln_bound and
    the GELU epilogue with one fp16 rounding.  L0 on both sides of the position tile and of 256."""
    from voicebox_pytorch_amd import _lib

    tile = _lib.call_value("vbx_hubert_conv0_ln_tile")
    B, k0, s0, eps = 2, 10, 5, 1e-5
    g = _gen(C + bias_on)
    w = (torch.randn(C, k0, generator=g) * 0.3).float()
    bias = (0.3 * torch.randn(C, generator=g)).float() if bias_on else None
    gam, bet = (0.75 + 0.5 * torch.rand(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()
    wd, gd, bd, biasd = w.to(dev), gam.to(dev), bet.to(dev), (bias.to(dev) if bias_on else None)
    for L0 in sorted({1, 2, 255, 256, 257, tile - 1, tile, tile + 1}):
        T = (L0 - 1) * s0 + k0 + 3  # three samples no frame reaches
        x = (100.0 + torch.randn(B, T, generator=g)).float()
        out = torch.full((B, L0, C), float("nan"), dtype=torch.float16, device=dev)
        _lib.call("vbx_hubert_conv0_ln", x.to(dev), wd, biasd, gd, bd, out, B, T, C, k0, s0, eps, _lib.current_stream())
        v = F.conv1d(x.double()[:, None], w.double()[:, None], bias.double() if bias_on else None, stride=s0).transpose(1, 2)  # [B, L0, C]
        assert v.shape[1] == L0
        dv = (k0 + 1) * U24 * F.conv1d(x.double().abs()[:, None], w.double().abs()[:, None], stride=s0).transpose(1, 2) + U24 * v.abs()
        z, dz = _ln_bound(v, dv, gam, bet, eps)
        ref = F.gelu(z)
        bound = _gelu_bound(z, ref, dz, True)
        err = (out.cpu().double() - ref).abs()
        print(f"conv0_ln C {C} bias {bias_on} L0 {L0}: worst err / bound {float((err / bound).max()):.3f}, max err {float(err.max()):.3e}")
        assert torch.isfinite(out).all() and (err <= bound).all(), (C, L0)


# ------------------------------------------------------------------------------------ the strided convolutions + LayerNorm
def _conv_ln_case(C, k, Lout, extra, bias_on, g, w, bias, gam, bet, eps=1e-5, B=2):
    from voicebox_pytorch_amd import _lib

    L = 2 * (Lout - 1) + k + extra
    x = torch.randn(B, L, C, generator=g).half()
    wp = w.permute(0, 2, 1).reshape(C, k * C).contiguous().to(dev)
    y = torch.full((B, Lout, C), float("nan"), dtype=torch.float16, device=dev)
    _lib.call("vbx_hubert_conv_ln", x.to(dev), wp, bias.to(dev) if bias_on else None, gam.to(dev), bet.to(dev), y, B, L, C, k, eps,
              _lib.current_stream())
    # the fp32 intermediate plus the row kernel: the same values through the same code, the SAME BITS (include/vbx.h)
    s32 = torch.full((B, Lout, C), float("nan"), device=dev)
    y2 = torch.full((B, Lout, C), float("nan"), dtype=torch.float16, device=dev)
    _lib.call("vbx_hubert_conv_f32", x.to(dev), wp, bias.to(dev) if bias_on else None, s32, B, L, C, k, _lib.current_stream())
    _lib.call("vbx_hubert_ln_gelu", s32, gam.to(dev), bet.to(dev), y2, B * Lout, C, eps, _lib.current_stream())
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), (C, k, Lout, "the pair and the fused kernel differ")
    s = F.conv1d(x.double().transpose(1, 2), w.double(), bias.double() if bias_on else None, stride=2).transpose(1, 2)  # [B, Lout, C]
    assert s.shape[1] == Lout
    ds = (k * C + 2) * U24 * F.conv1d(x.double().abs().transpose(1, 2), w.double().abs(), stride=2).transpose(1, 2) + U24 * s.abs()
    assert ((s32.cpu().double() - s).abs() <= ds).all()  # the intermediate itself: unrounded fp32 sums
    z, dz = _ln_bound(s, ds, gam, bet, eps)
    ref = F.gelu(z)
    return y.cpu().double(), s, ref, _gelu_bound(z, ref, dz, True)


@gpu
@pytest.mark.parametrize("bias_on", [True, False])
@pytest.mark.parametrize("C,k", [(32, 2), (32, 3), (16, 3), (512, 2), (512, 3)])
def test_strided_convolution_layernorm(C, k, bias_on):
    """ds = (k C + 2) 2^-24 sum |w a| for the product (+ 2^-24 |s| for the bias), _ln_bound over the C channels of each position, the
    GELU epilogue, one fp16 rounding.  Lout on both sides of the fused kernel's tile and of the pair's (vbx_hubert_conv_tile), the last tap
    on and one short of the last sample; the pair vbx_hubert_conv_f32 + vbx_hubert_ln_gelu must give the fused kernel's bits."""
    from voicebox_pytorch_amd import _lib

    tile, tile2 = _lib.call_value("vbx_hubert_conv_ln_tile", C, k), _lib.call_value("vbx_hubert_conv_tile", C, k)
    assert tile >= 16 and tile % 16 == 0
    g = _gen(C + k)
    w = (torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5).half()
    bias = (0.3 * torch.randn(C, generator=g)).float()
    gam, bet = (0.75 + 0.5 * torch.rand(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()
    for Lout in sorted({1, tile - 1, tile, tile + 1, tile2 - 1, tile2, tile2 + 1}):
        for extra in (0, 1):
            y, _, ref, bound = _conv_ln_case(C, k, Lout, extra, bias_on, g, w, bias, gam, bet)
            err = (y - ref).abs()
            assert torch.isfinite(y).all() and (err <= bound).all(), (C, k, Lout, extra, float((err / bound).max()))


@gpu
def test_strided_convolution_layernorm_takes_the_fp32_sums():
    """Per-channel sums of very unequal scale (weight rows over 2.5 decades: sums from 0.1 to 30) riding on a common offset of 200,
    where an fp16 ulp is 0.125: the norm must be taken from the fp32 sums.  The same norm from fp16-ROUNDED sums (computed here in
    fp64) breaks the bound the kernel has to meet on most elements, so the case can tell."""
    C, k = 32, 3
    g = _gen(9)
    scale = 10.0 ** (torch.rand(C, generator=g) * 2.5 - 1.0)
    w = (torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5 * scale[:, None, None]).half()
    bias = (200.0 + 0.3 * torch.randn(C, generator=g)).float()
    gam, bet = (0.75 + 0.5 * torch.rand(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()
    y, s, ref, bound = _conv_ln_case(C, k, 40, 0, True, g, w, bias, gam, bet)
    err = (y - ref).abs()
    print(f"unequal scales: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    rounded = F.gelu(F.layer_norm(s.half().double(), (C,), gam.double(), bet.double(), 1e-5))
    worse = (rounded - ref).abs() / bound
    print(f"  the norm of fp16-rounded sums: worst err / bound {float(worse.max()):.1f}, {float((worse > 1).float().mean()) * 100:.0f} % of elements over it")
    assert (worse > 1).float().mean() > 0.5


@gpu
def test_pair_route_on_both_sides_of_its_threshold():
    """vbx_hubert_conv_ln_route: the pair where the fused tile is the smaller one AND the grid is more than 512 workgroups.  Both ways at
    a shape on each side, bit-equal and inside the bound (_conv_ln_case runs both); the module follows the route."""
    from voicebox_pytorch_amd import _lib

    C, k = 512, 3
    tile, tile2 = _lib.call_value("vbx_hubert_conv_ln_tile", C, k), _lib.call_value("vbx_hubert_conv_tile", C, k)
    route = lambda B, Lout: _lib.call_value("vbx_hubert_conv_ln_route", B, 2 * (Lout - 1) + k, C, k)
    assert route(1, 1) == 0 and _lib.call_value("vbx_hubert_conv_ln_route", 8, 31999, 32, 3) == 0  # equal tiles at 32 channels: always fused
    if tile < tile2:
        assert route(2, 256 * tile) == 0 and route(2, 256 * tile + 1) == 1 and route(8, 15999) == 1
    g = _gen(12)
    w = (torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5).half()
    bias = (0.3 * torch.randn(C, generator=g)).float()
    gam, bet = (0.75 + 0.5 * torch.rand(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()
    for Lout in (256 * tile, 256 * tile + 1):
        y, _, ref, bound = _conv_ln_case(C, k, Lout, 0, True, g, w, bias, gam, bet)
        assert ((y - ref).abs() <= bound).all(), Lout


# ------------------------------------------------------------------------------------ wave normalisation
def _normalize_bound(x, lens, eps):
    """A = max |x - mean| of the row, u = 2^-24.  Every d = x - K has |d| <= 2 A.  S1 of a chunk: <= 25 additions (16 in a thread, the
    6-level tree, the four waves) -> |dmean| <= 64 u A with the rounding of each d.  S2: 28 u sum d^2 <= 112 u A^2 per sample; through
    S1^2 / n another 200 u A^2; through the chunk means 208 u A^2: |dvar| <= 520 u A^2.  The combination and the application run in
    fp64 and the result is rounded once: |dy| <= rstd 64 u A + |y| 520 u A^2 / (2 (var + eps)) + 4 u |y|."""
    ref = LR.normalize(x, lens, eps)
    bound = torch.zeros_like(ref)
    for b in range(x.shape[0]):
        l = x.shape[1] if lens is None else lens[b]
        r = x[b, :l].double()
        A, var = (r - r.mean()).abs().max(), r.var(unbiased=False)
        bound[b, :l] = 64 * U24 * A / torch.sqrt(var + eps) + ref[b, :l].abs() * (520 * U24 * A * A / (2 * (var + eps)) + 4 * U24)
    return ref, bound


@gpu
def test_wave_normalize():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    chunk = _lib.call_value("vbx_wave_normalize_chunk")
    g = _gen(3)
    for T in (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 17):
        x = (100.0 + torch.randn(3, T, generator=g)).float()  # mean 100, std 1: a naive fp32 sum of squares loses the variance
        y = vbx.normalize_wave(x.to(dev))
        ref, bound = _normalize_bound(x, None, 1e-7)
        err = (y.cpu().double() - ref).abs()
        assert y.dtype == torch.float32 and y.shape == x.shape and (err <= bound).all(), (T, float(err.max()))
        if T == 1:
            assert (y == 0).all()  # defined: 0 / sqrt(eps)
        else:
            print(f"normalize T {T}: worst err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}, max err {float(err.max()):.2e}")
        assert torch.equal(vbx.normalize_wave(x.to(dev)), y)  # a rerun
        assert torch.equal(vbx.normalize_wave(x[1:2].to(dev))[0], y[1])  # a row alone
    y2 = vbx.normalize_wave(x.to(dev), eps=1e-2)
    assert ((y2.cpu().double() - LR.normalize(x, None, 1e-2)).abs() <= _normalize_bound(x, None, 1e-2)[1]).all() and not torch.equal(y2, y)


@gpu
def test_wave_normalize_keeps_mean_and_rstd_in_fp64():
    """include/vbx.h: the mean and rstd stay fp64 and (x - mean) * rstd is formed in fp64.  Rows at mean ~1000 with std 0.01: the mean
    rounded to fp32 is off by up to 1000 * 2^-24 = 6e-5, which times rstd = 100 is 6e-3 of a unit-variance sample, above the bound of
    _normalize_bound (about 1e-3 here) -- shown on the CPU for these rows, so the case can tell.  (rstd in fp32 would cost 2^-24 |y|,
    the size of the final rounding: no test can tell that.)"""
    import voicebox_pytorch_amd as vbx

    g = _gen(6)
    x = (torch.tensor([1000.3, 777.7, 1234.5, 1500.1])[:, None].double() + 0.01 * torch.randn(4, 6000, generator=g, dtype=torch.float64)).float()
    ref, bound = _normalize_bound(x, None, 1e-7)
    xd = x.double()
    mean32 = xd.mean(1, keepdim=True).float().double()
    coarse = (xd - mean32) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-7)
    over = ((coarse - ref).abs() > bound).float().mean(1)
    print("an fp32 mean: share of samples over the bound per row", [f"{float(v):.2f}" for v in over])
    assert (over > 0.5).sum() >= 2  # the rounding of a mean to fp32 can be small by chance in a row, not in most of four
    err = (vbx.normalize_wave(x.to(dev)).cpu().double() - ref).abs()
    print(f"normalize at mean 1000 / std 0.01: worst err / bound {float((err / bound).max()):.3f}, max err {float(err.max()):.2e}")
    assert (err <= bound).all()


@gpu
def test_wave_normalize_lens():
    """own-sample statistics, zeros past len_b whatever the padding holds, a row alone bit-equal; lengths on both sides of the chunk"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    chunk = _lib.call_value("vbx_wave_normalize_chunk")
    lens = [2 * chunk + 5, chunk + 1, chunk, chunk - 1, 2, 1]
    T = lens[0]
    x = (torch.randn(len(lens), T, generator=_gen(4)) * 0.3 + torch.arange(len(lens))[:, None] * 7.0).float()
    y = vbx.normalize_wave(x.to(dev), lens=lens)
    ref, bound = _normalize_bound(x, lens, 1e-7)
    assert ((y.cpu().double() - ref).abs() <= bound).all()
    for b, l in enumerate(lens):
        assert torch.equal(y[b, :l], vbx.normalize_wave(x[b:b + 1, :l].contiguous().to(dev))[0]), b
        assert (y[b, l:].view(torch.int32) == 0).all(), b
    for fill in (float("nan"), float("inf"), 1e30):
        xn = x.clone()
        for b, l in enumerate(lens):
            xn[b, l:] = fill
        assert torch.equal(vbx.normalize_wave(xn.to(dev), lens=lens).view(torch.int32), y.view(torch.int32))
    assert torch.equal(vbx.normalize_wave(x.to(dev), lens=torch.tensor(lens, device=dev)), y)
    assert torch.equal(vbx.normalize_wave(x.to(dev), lens=[T] * len(lens)), vbx.normalize_wave(x.to(dev)))
    wild = torch.tensor([T + 9, -4, 0, 2 ** 31 - 1, 2, 1], device=dev)  # a device tensor is clamped into 1 .. T
    yw = vbx.normalize_wave(x.to(dev), lens=wild)
    assert torch.isfinite(yw).all() and torch.equal(yw[0], vbx.normalize_wave(x[:1].to(dev))[0]) and (yw[1] == 0).all()


# ------------------------------------------------------------------------------------ the whole network
def _model(cfg, sd, output_layer, centers, **kw):
    import voicebox_pytorch_amd as vbx

    m = vbx.HubertLargeWithKmeans(**cfg, output_layer=output_layer, codebook_size=centers.shape[0], **kw)
    m.load_state_dict(sd)
    m.set_cluster_centers(centers)
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def _small(output_layer=4, normalize_wave=False):
    return _model(LR.LSMALL, LR.small_state_dict(), output_layer, LR.codebook("LSMALL", 0, 4, 64), normalize_wave=normalize_wave)


@functools.lru_cache(maxsize=None)
def _small_case(T, layer):
    wave = R.make_wave(2, T, 20 + T % 97)
    sd = LR.small_state_dict()
    with torch.no_grad():
        return wave, LR.features(sd, LR.LSMALL, wave, layer), LR.features(sd, LR.LSMALL, wave, layer, emulate=True)


@gpu
@pytest.mark.parametrize("layer", [2, 4])
@pytest.mark.parametrize("T", [400, 719, 720, 5000])
def test_features_small(T, layer):
    """layer 2 of 4: the un-normalised stream; layer 4 of 4: encoder.layer_norm applied"""
    tol, _ = LR.tolerance_small(layer)
    m = _small(layer)
    wave, ref, emu = _small_case(T, layer)
    h = m.features(wave.to(dev))
    assert h.shape == ref.shape == (2, R.frames_of(T, LR.LSMALL), 128) and h.dtype == torch.float32
    a, b = R.movement(h.cpu().double(), ref), R.movement(h.cpu().double(), emu)
    print(f"LSMALL T {T} layer {layer}: vs fp64 {a:.3e}, vs emulated {b:.3e}, tolerance {tol:.3e}")
    assert a < tol and b < tol
    assert torch.equal(m.features(wave.to(dev)), h)  # a rerun
    assert torch.equal(m.features(wave[1:].to(dev))[0], h[1])  # a row alone
    ids = m(wave.to(dev))
    assert ids.dtype == torch.int64 and ids.shape == h.shape[:2] and torch.equal(ids, m.assign(h))
    assert torch.equal(m(wave[:, None].to(dev)), ids)  # [B, 1, T]


@gpu
def test_features_small_without_conv_bias():
    tol, _ = LR.tolerance_small(4)
    sd, wave = LR.small_state_dict(conv_bias=False), R.make_wave(2, 5000, 23)
    m = _model(LR.LSMALL, sd, 4, torch.randn(64, 128, generator=_gen(1)), conv_bias=False)
    with torch.no_grad():
        ref = LR.features(sd, LR.LSMALL, wave, 4)
    a = R.movement(m.features(wave.to(dev)).cpu().double(), ref)
    assert a < tol, a


@gpu
def test_normalize_wave_keyword():
    """normalize_wave=True is normalize_wave() of the prepared wave, then the same network"""
    import voicebox_pytorch_amd as vbx

    tol, _ = LR.tolerance_small(4)
    m, mn = _small(4), _small(4, True)
    wave = (R.make_wave(2, 5000, 8) * 0.05 + 0.4)  # quiet, with a DC offset: normalisation changes everything
    wd = wave.to(dev)
    h = mn.features(wd)
    assert torch.equal(h, m.features(vbx.normalize_wave(wd))) and not torch.equal(h, m.features(wd))
    with torch.no_grad():
        ref = LR.features(LR.small_state_dict(), LR.LSMALL, LR.normalize(wave), 4)
    a = R.movement(h.cpu().double(), ref)
    print(f"LSMALL normalize_wave: vs fp64 {a:.3e}, tolerance {tol:.3e}")
    assert a < tol
    # after resampling and curtailing: the statistics of the samples the network sees
    mm = _model(LR.LSMALL, LR.small_state_dict(), 4, m.cluster_centers.cpu(), normalize_wave=True, seq_len_multiple_of=320)
    w24 = R.make_wave(2, 9000, 4, rate=24000).to(dev)
    prepared = vbx.resample(w24, 24000, 16000)[:, :6000 // 320 * 320].contiguous()
    assert torch.equal(mm.features(w24, input_sample_hz=24000), m.features(vbx.normalize_wave(prepared)))


@gpu
@pytest.mark.parametrize("layer", [6, 3])
def test_features_large_widths(layer):
    """hidden 1024, 16 heads, intermediate 4096, 512 channels, 128 taps in 16 groups; six layers: layer 6 takes the final norm"""
    tol, _ = LR.tolerance_small(4 if layer == 6 else 2)
    sd, wave = LR.large6_state_dict(), R.make_wave(1, 16000, 31)
    with torch.no_grad():
        ref = LR.features(sd, LR.LARGE6, wave, layer)
    m = _model(LR.LARGE6, sd, layer, torch.randn(500, 1024, generator=_gen(1)))
    h = m.features(wave.to(dev))
    assert h.shape == (1, 49, 1024)
    a = R.movement(h.cpu().double(), ref)
    print(f"LARGE6 T 16000 layer {layer}: vs fp64 {a:.3e}, tolerance {tol:.3e}")
    assert a < tol
    assert torch.equal(m(wave.to(dev)), m.assign(h))


@gpu
def test_code_agreement_small():
    """at most 5 % of 198 frames carry a code other than the fp64 restatement's argmin, and every differing frame still satisfies the
    k-means contract on the device's OWN features (the cap of tests/test_hubert_gpu.py)"""
    m = _small()
    wave = R.make_wave(2, 400 + 320 * 98, 77)
    with torch.no_grad():
        ref = LR.features(LR.small_state_dict(), LR.LSMALL, wave, 4)
    c = m.cluster_centers.cpu()
    want, _ = R.kmeans_assign(ref, c)
    h, ids = m.features(wave.to(dev)), m(wave.to(dev)).cpu()
    differ = ids != want
    print(f"code agreement LSMALL: {int(differ.sum())} of {differ.numel()} frames differ")
    assert differ.numel() == 198 and differ.float().mean() <= 0.05
    ok, _ = _contract_ok(h.cpu().reshape(-1, 128), c, ids.reshape(-1))
    assert ok.all()


def _launches(m, wave):
    from voicebox_pytorch_amd import _lib

    n, call, gemm = [0], _lib.call, type(m)._gemm
    count = lambda f: (lambda *a, **k: (n.__setitem__(0, n[0] + 1), f(*a, **k))[1])
    _lib.call, type(m)._gemm = count(call), staticmethod(count(gemm))
    try:
        m(wave)
    finally:
        _lib.call, type(m)._gemm = call, staticmethod(gemm)
    return n[0]


@gpu
def test_output_layer_runs_only_its_layers():
    """output_layer = 2 of 4: layers 3 and 4 are loaded, never packed or launched -- the bits and the launches of a model that HAS
    only the layers up to 2 and is asked for the same tensor.  In the large form a 2-layer model's hidden_states[2] is its LAST state
    and carries encoder.layer_norm, which hidden_states[2] of 4 does not: so the twin here has three layers (same bits, same
    launches), and the 2-layer model is one launch more, its features bit-equal to vbx_hubert_layernorm of the un-normalised ones."""
    from voicebox_pytorch_amd import _lib

    wave = R.make_wave(2, 5000, 3).to(dev)
    m4 = _small(2)
    assert len(m4._cached(m4._pack)["layers"]) == 2
    sd = LR.small_state_dict()
    sd3 = {k: v for k, v in sd.items() if not k.startswith("encoder.layers.3.")}
    sd2 = {k: v for k, v in sd3.items() if not k.startswith("encoder.layers.2.")}
    c = m4.cluster_centers.cpu()
    m3 = _model(dict(LR.LSMALL, num_hidden_layers=3), sd3, 2, c)
    m2 = _model(dict(LR.LSMALL, num_hidden_layers=2), sd2, 2, c)
    h4 = m4.features(wave)
    assert torch.equal(h4, m3.features(wave)) and torch.equal(m4(wave), m3(wave))
    n4 = _launches(m4, wave)
    assert n4 == _launches(m3, wave) == 1 + 6 + 3 + 2 * 8 + 1  # eight launches per layer
    assert _launches(m2, wave) == n4 + 1 and _launches(_small(4), wave) == n4 + 2 * 8 + 1
    normed = torch.empty_like(h4)
    _lib.call("vbx_hubert_layernorm", h4.contiguous(), m2.encoder.layer_norm.weight, m2.encoder.layer_norm.bias, normed, None, h4.shape[0] * h4.shape[1],
              128, 1e-5, _lib.current_stream())
    assert torch.equal(m2.features(wave), normed)


# ------------------------------------------------------------------------------------ lens=
LENS_T, LENS = 5000, (5000, 3333, 719)


@gpu
@pytest.mark.parametrize("normalize", [False, True])
def test_rows_under_lens_are_the_rows_alone(normalize):
    m = _small(4, normalize)
    lens = list(LENS)
    wave = R.make_wave(3, LENS_T, 51)
    if normalize:
        wave = wave * 0.1 + 0.3
    frames = [R.frames_of(l, LR.LSMALL) for l in lens]
    N = frames[0]
    want = m.gemm_routes(3 * N)
    for f in frames:
        assert m.gemm_routes(f) == want, f"vbx_gemm_route answers differently for {3 * N} rows and for {f}: no bit claim stands"
    assert m.frame_lens(lens) == frames
    wd = wave.to(dev)
    h, ids = m.features(wd, lens=lens), m(wd, lens=lens)
    assert h.shape == (3, N, 128) and ids.shape == (3, N)
    tol, _ = LR.tolerance_small(4)
    sd = LR.small_state_dict()
    for b, (l, f) in enumerate(zip(lens, frames)):
        one = wd[b:b + 1, :l].contiguous()
        assert torch.equal(h[b, :f], m.features(one)[0]) and torch.equal(ids[b, :f], m(one)[0]), b
        assert (h[b, f:].view(torch.int32) == 0).all() and (ids[b, f:] == 0).all(), b
        row = wave[b:b + 1, :l]
        with torch.no_grad():
            ref = LR.features(sd, LR.LSMALL, LR.normalize(row) if normalize else row, 4)
        move = R.movement(h[b, :f].cpu().double(), ref[0])
        print(f"LSMALL normalize {normalize} row {b} len {l} ({f} frames): vs fp64 of the row alone {move:.3e}, tolerance {tol:.3e}")
        assert move < tol
    for fill in ("noise", "nan", "inf"):  # what lies behind the lengths is never read into a live frame
        wn = wave.clone()
        for b, l in enumerate(lens):
            wn[b, l:] = {"noise": 5.0 * torch.randn(LENS_T - l, generator=_gen(b)), "nan": float("nan"), "inf": float("inf")}[fill]
        assert torch.equal(m.features(wn.to(dev), lens=lens).view(torch.int32), h.view(torch.int32)), fill
        assert torch.equal(m(wn.to(dev), lens=lens), ids), fill
    assert torch.equal(m.features(wd, lens=torch.tensor(lens, device=dev)), h)
    assert torch.equal(m.features(wd, lens=[LENS_T] * 3), m.features(wd))  # full lengths are the call without lengths


# ------------------------------------------------------------------------------------ the wrapper, fit_kmeans, mark_weights_dirty
@gpu
def test_wrapper_computes_semantic_ids_from_the_wave():
    """wrapper(wave) with wav2vec= the large tokenizer is wrapper(wave, semantic_token_ids=tok(resample(wave))) bit for bit"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    torch.manual_seed(3)
    tok = _small()
    w_tok = _wrapper(wav2vec=tok)
    w_ids = _wrapper(state={k: v.detach().cpu().clone() for k, v in w_tok.voicebox.state_dict().items()})
    wave = R.make_wave(2, 9600, 8, rate=24000).to(dev)
    ids = tok(vbx.resample(wave, 24000, 16000))
    assert ids.shape == (2, 19) and len(ids.unique()) > 4
    draws = _draws((2, 61, 100))
    with rng_override(**draws):
        a = w_tok(wave)
    with rng_override(**draws):
        b = w_ids(wave, semantic_token_ids=ids)
    with rng_override(**draws):
        e = w_ids(wave, semantic_token_ids=ids.flip(1).contiguous())
    assert torch.isfinite(a) and torch.equal(a.detach(), b.detach()) and not torch.equal(a.detach(), e.detach())


@gpu
def test_fit_kmeans_sets_a_codebook_that_assign_honours():
    m = _model(LR.LSMALL, LR.small_state_dict(), 4, torch.zeros(64, 128))
    batches = [R.make_wave(2, 8000, 60).to(dev), (R.make_wave(2, 8000, 61).to(dev), [8000, 5000])]
    km = m.fit_kmeans(batches, n_clusters=16, seed=1)
    c = m.cluster_centers.cpu()
    assert m.codebook_size == 16 and c.shape == (16, 128) and torch.isfinite(c).all() and torch.equal(c, km.cluster_centers_.cpu())
    wave = R.make_wave(2, 8000, 62).to(dev)
    h, ids = m.features(wave), m(wave).cpu()
    ok, _ = _contract_ok(h.cpu().reshape(-1, 128), c, ids.reshape(-1))
    assert ok.all() and len(ids.unique()) > 2 and int(ids.max()) < 16


@gpu
def test_mark_weights_dirty_reaches_the_convolution_norms():
    m = _small()
    wave = R.make_wave(1, 2000, 9).to(dev)
    h0 = m.features(wave)
    p = m.feature_extractor.conv_layers[3].layer_norm.weight
    old = p.data.clone()
    p.data.mul_(1.5)
    m.mark_weights_dirty()
    assert not torch.equal(m.features(wave), h0)
    p.data.copy_(old)
    m.mark_weights_dirty()
    assert torch.equal(m.features(wave), h0)


@gpu
def test_limits_on_the_device():
    from voicebox_pytorch_amd import _lib

    m = _small()
    with pytest.raises(NotImplementedError, match="shorter than one frame"):
        m(torch.zeros(1, 399, device=dev))
    with pytest.raises(NotImplementedError, match="mask"):
        m(torch.zeros(1, 800, device=dev), attention_mask=torch.ones(1, 800, device=dev))
    with pytest.raises(_lib.VbxError):
        m(torch.zeros(1, 800))
    with pytest.raises(ValueError, match=r"lens\[1\] = 399"):
        m(torch.zeros(2, 800, device=dev), lens=[800, 399])
    with pytest.raises(_lib.VbxError, match="multiple of 16"):  # the entry points check their own limits
        _lib.call("vbx_hubert_conv0_ln", torch.zeros(1, 100, device=dev), torch.zeros(24, 10, device=dev), None, torch.zeros(24, device=dev),
                  torch.zeros(24, device=dev), torch.zeros(1, 19, 24, dtype=torch.float16, device=dev), 1, 100, 24, 10, 5, 1e-5, _lib.current_stream())
