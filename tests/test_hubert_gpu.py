"""voicebox_pytorch_amd.HubertWithKmeans on the device (csrc/hubert.hip) against the restatement tests/hubert_ref.py, which
tests/test_hubert_cpu.py pins to transformers.HubertModel.

Single kernels: fp64 on the same operands under DERIVED per-element bounds of the family's form.  With ds = (K + 2) * 2^-24 * sum |w a|
(any fp32 summation order of K products), the epilogue y = gelu(s) adds: |gelu'| <= 1.13 times ds; libm's erff, the argument's
scaling, 1 + erf and the two multiplications, each within an fp32 ulp or two of |s| or |y| -- c = 8 covers them:
8 * 2^-24 * (|s| + |y|); 2^-11 |y| + 2^-25 where y is stored as fp16.  The bounds of GroupNorm and the LayerNorms are derived where
they are used.
Whole network: max |delta| / RMS against fp64 and against the emulated restatement, inside the tolerance MEASURED by
hubert_ref.tolerance_small() -- a tenth of the smallest planted fault's movement (profiles/hubert_parity.txt), not a number fixed here."""
import functools

import pytest
import torch
import torch.nn.functional as F

import hubert_ref as R

gpu = pytest.mark.gpu
dev = "cuda"
U24, U11 = 2.0 ** -24, 2.0 ** -11


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _gelu_bound(s, y, ds, f16_out):
    b = 1.13 * ds + 8 * U24 * (s.abs() + y.abs())
    return b + (U11 * y.abs() + 2.0 ** -25 if f16_out else U24 * y.abs())


def _model(cfg, sd, output_layer, centers):
    import voicebox_pytorch_amd as vbx

    m = vbx.HubertWithKmeans(**cfg, output_layer=output_layer, codebook_size=centers.shape[0])
    m.load_state_dict(sd)
    m.set_cluster_centers(centers)
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def _small(output_layer=4):
    return _model(R.SMALL, R.small_state_dict(), output_layer, R.codebook("SMALL", 0, 4, 64))


# ------------------------------------------------------------------------------------ conv0 + GroupNorm
@gpu
@pytest.mark.parametrize("L0", [1, 2, 255, 256, 257])
def test_conv0_groupnorm(L0):
    """A row with a large DC offset (mean 100, std 1): a naive fp32 sum of squares loses the variance.  Bound: dv = (k0 + 1) 2^-24
    sum |w x| per element; the mean of a row inherits at most max dv plus an fp32 rounding of itself; var = mean((v - mean)^2) moves
    by at most 2 std max dv relatively 2 max dv / std, so rstd by max dv * rstd (+ 4 ulps for the fp64 -> fp32 roundings and sqrt);
    z = (v - mean) rstd gamma + beta: rstd |gamma| (dv + dmean) + |z - beta| drstd + 4 ulps of |z| + |beta|; then the GELU epilogue."""
    from voicebox_pytorch_amd import _lib

    B, C, k0, s0, eps = 2, 32, 10, 5, 1e-5
    T = (L0 - 1) * s0 + k0 + 3  # three samples no frame reaches
    g = _gen(L0)
    x = (100.0 + torch.randn(B, T, generator=g)).float()
    w = (torch.randn(C, k0, generator=g) * 0.3).float()
    gam, bet = (0.75 + 0.5 * torch.rand(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()
    xd, wd = x.to(dev), w.to(dev)
    chunks = _lib.call_value("vbx_hubert_conv0_chunks", L0)
    rec, stats = torch.empty(B, chunks, C, 3, device=dev), torch.empty(B, C, 2, device=dev)
    st = _lib.current_stream()
    _lib.call("vbx_hubert_conv0_stats", xd, wd, rec, stats, B, T, C, k0, s0, eps, st)
    out = torch.empty(B, L0, C, dtype=torch.float16, device=dev)
    _lib.call("vbx_hubert_conv0_apply", xd, wd, stats, gam.to(dev), bet.to(dev), out, B, T, C, k0, s0, st)
    out = out.cpu().double()
    v = F.conv1d(x.double()[:, None], w.double()[:, None], stride=s0)  # [B, C, L0]
    assert v.shape[2] == L0
    dv = (k0 + 1) * U24 * F.conv1d(x.double().abs()[:, None], w.double().abs()[:, None], stride=s0)
    mean, var = v.mean(2, keepdim=True), v.var(2, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (v - mean) * rstd * gam.double()[:, None] + bet.double()[:, None]
    ref = F.gelu(z)
    dvm = dv.amax(2, keepdim=True)
    dmean = dvm + U24 * mean.abs()
    drstd = dvm * rstd + 4 * U24
    dz = rstd * gam.double().abs()[:, None] * (dv + dmean) + (z - bet.double()[:, None]).abs() * drstd + 4 * U24 * (z.abs() + bet.double().abs()[:, None])
    bound = _gelu_bound(z, ref, dz, True)
    err = (out.transpose(1, 2) - ref).abs()
    print(f"conv0 L0 {L0}: worst err / bound {float((err / bound).max()):.3f}, max err {float(err.max()):.3e}")
    assert torch.isfinite(out).all() and (err <= bound).all()
    # the statistics themselves against fp64: far inside what a naive fp32 sum of x^2 at mean 100 gives (~1e-2 relative)
    if L0 > 2:
        sm = stats.cpu().double()
        assert ((sm[..., 1] - rstd[..., 0]).abs() <= (drstd[..., 0] * rstd[..., 0])).all()


# ------------------------------------------------------------------------------------ the strided convolutions
@gpu
@pytest.mark.parametrize("C,k", [(32, 2), (32, 3), (16, 3), (512, 2), (512, 3)])
def test_strided_convolution(C, k):
    from voicebox_pytorch_amd import _lib

    tile = _lib.call_value("vbx_hubert_conv_tile", C, k)
    g = _gen(C + k)
    w = (torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5).half()
    wp = w.permute(0, 2, 1).reshape(C, k * C).contiguous().to(dev)
    for Lout in (1, tile - 1, tile, tile + 1):
        for extra in (0, 1):  # the last tap lands on the last sample, and one short of it
            L, B = 2 * (Lout - 1) + k + extra, 2
            x = torch.randn(B, L, C, generator=g).half()
            y = torch.empty(B, Lout, C, dtype=torch.float16, device=dev)
            _lib.call("vbx_hubert_conv", x.to(dev), wp, y, B, L, C, k, _lib.current_stream())
            s = F.conv1d(x.double().transpose(1, 2), w.double(), stride=2)
            assert s.shape[2] == Lout
            ds = (k * C + 2) * U24 * F.conv1d(x.double().abs().transpose(1, 2), w.double().abs(), stride=2)
            ref = F.gelu(s)
            err = (y.cpu().double().transpose(1, 2) - ref).abs()
            assert (err <= _gelu_bound(s, ref, ds, True)).all(), (C, k, Lout, extra, float(err.max()))


# ------------------------------------------------------------------------------------ the positional convolution
@gpu
@pytest.mark.parametrize("D,G,k,Ns", [(128, 4, 16, (1, 2, 7, 8, 9, 17, 127, 128, 129)), (768, 16, 128, (1, 63, 64, 65, 127, 128, 129))])
def test_positional_convolution(D, G, k, Ns):
    from voicebox_pytorch_amd import _lib

    tile = _lib.call_value("vbx_hubert_posconv_tile", D // G, k)
    assert {tile - 1, tile, tile + 1} <= set(Ns)  # both sides of the tile
    g = _gen(D + k)
    w = (torch.randn(D, D // G, k, generator=g) * (1.0 / (k * D // G)) ** 0.5).half()
    bias = (0.3 * torch.randn(D, generator=g)).float()
    wp = w.permute(0, 2, 1).reshape(D, -1).contiguous().to(dev)
    for N in Ns:
        B = 2
        x = torch.randn(B, N, D, generator=g).float()
        y = torch.empty(B, N, D, device=dev)
        _lib.call("vbx_hubert_posconv", x.to(dev), wp, bias.to(dev), y, B, N, D, G, k, _lib.current_stream())
        a = x.half().double().transpose(1, 2)
        s = F.conv1d(a, w.double(), bias.double(), padding=k // 2, groups=G)[..., :-1]
        ds = (k * D // G + 3) * U24 * (F.conv1d(a.abs(), w.double().abs(), padding=k // 2, groups=G)[..., :-1] + bias.double().abs()[:, None])
        ge = F.gelu(s)
        ref = ge + x.double().transpose(1, 2)
        bound = _gelu_bound(s, ge, ds, False) + U24 * ref.abs()
        err = (y.cpu().double().transpose(1, 2) - ref).abs()
        assert (err <= bound).all(), (D, N, float(err.max()))


# ------------------------------------------------------------------------------------ head split and LayerNorms
@gpu
def test_split_heads_bit_equal():
    from voicebox_pytorch_amd import _lib

    B, N, H = 2, 37, 3
    D = 64 * H
    qkv = torch.randn(B * N, 3 * D, generator=_gen(5)).float()
    pre = _lib.lib().vbx_attn_q_prescale(64 ** -0.5)
    q, k, v = (torch.empty(B, H, N, 64, dtype=torch.float16, device=dev) for _ in range(3))
    _lib.call("vbx_hubert_split_heads", qkv.to(dev), q, k, v, B, N, H, pre, _lib.current_stream())
    t = qkv.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    assert torch.equal(q.cpu(), (t[0] * torch.tensor(pre, dtype=torch.float32)).half())
    assert torch.equal(k.cpu(), t[1].half()) and torch.equal(v.cpu(), t[2].half())


@gpu
@pytest.mark.parametrize("D", [64, 1280])
def test_layernorms(D):
    """fp32 two-pass LayerNorm: the mean of D terms carries (D / 64 + 7) ulps of max |x| (64 lane sums of D / 64 terms, a 6-level tree,
    the division), the deviations inherit it, rstd moves relatively by as many ulps; the affine adds two roundings:
    bound = 2^-24 * [(D / 64 + 16) * rstd |gamma| max |x| + (D / 64 + 16) |z - beta| + 4 (|y| + |beta|)] (+ 2^-11 |y| + 2^-25 as fp16)."""
    from voicebox_pytorch_amd import _lib

    M, eps, g = 9, 1e-5, _gen(D)
    x = (torch.randn(M, D, generator=g) * 2 + 1.5).float()
    gam, bet = (0.75 + 0.5 * torch.rand(D, generator=g)).float(), (0.2 * torch.randn(D, generator=g)).float()
    st = _lib.current_stream()

    def check(xin, y32, y16):
        xd = xin.double()
        ref = F.layer_norm(xd, (D,), gam.double(), bet.double(), eps)
        rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
        c = D / 64 + 16
        b32 = U24 * (c * rstd * gam.double().abs() * xd.abs().amax(1, keepdim=True) + c * (ref - bet.double()).abs() + 4 * (ref.abs() + bet.double().abs()))
        if y32 is not None:
            assert ((y32.cpu().double() - ref).abs() <= b32).all()
        assert ((y16.cpu().double() - ref).abs() <= b32 + U11 * ref.abs() + 2.0 ** -25).all()
        if y32 is not None:
            assert torch.equal(y16.cpu(), y32.cpu().half())  # the copy is the fp32 row rounded once

    y32, y16 = torch.empty(M, D, device=dev), torch.empty(M, D, dtype=torch.float16, device=dev)
    _lib.call("vbx_hubert_layernorm", x.to(dev), gam.to(dev), bet.to(dev), y32, y16, M, D, eps, st)
    check(x, y32, y16)
    x16 = x.half()
    _lib.call("vbx_hubert_layernorm16", x16.to(dev), gam.to(dev), bet.to(dev), y16, M, D, eps, st)
    check(x16, None, y16)


# ------------------------------------------------------------------------------------ k-means
def _assign(h, c):
    from voicebox_pytorch_amd import _lib

    ids = torch.empty(h.shape[0], dtype=torch.int64, device=dev)
    _lib.call("vbx_kmeans_assign", h.to(dev), c.to(dev), ids, h.shape[0], h.shape[1], c.shape[0], _lib.current_stream())
    return ids.cpu()


def _contract_ok(h, c, ids):
    """d(code) - min d <= (D + 2) 2^-23 (|h| + max |c|)^2 per frame, both distances in fp64"""
    best, d = R.kmeans_assign(h, c)
    slack = d.gather(1, ids[:, None])[:, 0] - d.min(1).values
    return slack <= R.kmeans_bound(h, c), best


@gpu
@pytest.mark.parametrize("D,K", [(128, 64), (768, 500), (1024, 4096)])
def test_kmeans_assign(D, K):
    g = _gen(D + K)
    c = torch.randn(K, D, generator=g).float()
    c[K // 2 + 3] = c[5]          # duplicate rows: the lowest index must win
    c[K - 1] = c[K // 3]
    c[7] = c[6]
    c[7, 0] = torch.nextafter(c[6, 0], torch.tensor(float("inf")))  # a near tie: one coordinate one fp32 ulp apart
    for N in (1, 33, 129):
        h = (c[torch.randint(0, K, (N,), generator=g)] + 0.3 * torch.randn(N, D, generator=g)).float()
        h[0] = c[5] + 0.01 * torch.randn(D, generator=g)
        if N > 2:
            h[1], h[2] = c[K // 3] + 0.01 * torch.randn(D, generator=g), (c[6] + c[7]) / 2 + 0.01 * torch.randn(D, generator=g)
        ids = _assign(h, c)
        ok, best = _contract_ok(h, c, ids)
        assert ((ids >= 0) & (ids < K)).all() and ok.all(), (N, int((~ok).sum()))
        assert ids[0] == 5
        if N > 2:
            assert ids[1] == K // 3 and ids[2] in (6, 7)
            assert torch.equal(_assign(h[3:4], c), ids[3:4]) and torch.equal(_assign(h[N - 1:], c), ids[N - 1:])  # a row alone
        assert torch.equal(_assign(h, c), ids)  # a rerun


# ------------------------------------------------------------------------------------ the whole network
@functools.lru_cache(maxsize=None)
def _small_case(T):
    wave = R.make_wave(2, T, 20 + T % 97)
    with torch.no_grad():
        return wave, R.features(R.small_state_dict(), R.SMALL, wave, 4), R.features(R.small_state_dict(), R.SMALL, wave, 4, emulate=True)


@gpu
@pytest.mark.parametrize("T", [400, 719, 720, 5000, 41360])
def test_features_small(T):
    tol, _ = R.tolerance_small()
    m = _small()
    wave, ref, emu = _small_case(T)
    h = m.features(wave.to(dev))
    assert h.shape == ref.shape == (2, R.frames_of(T, R.SMALL), 128) and h.dtype == torch.float32
    a, b = R.movement(h.cpu().double(), ref), R.movement(h.cpu().double(), emu)
    print(f"SMALL T {T}: vs fp64 {a:.3e}, vs emulated {b:.3e}, tolerance {tol:.3e}")
    assert a < tol and b < tol
    assert torch.equal(m.features(wave.to(dev)), h)  # a rerun
    assert torch.equal(m.features(wave[1:].to(dev))[0], h[1])  # a row alone
    ids = m(wave.to(dev))
    assert ids.dtype == torch.int64 and ids.shape == h.shape[:2] and torch.equal(ids, m.assign(h))
    assert torch.equal(m(wave[:, None].to(dev)), ids)  # [B, 1, T]


@gpu
def test_features_base_widths():
    tol, _ = R.tolerance_small()
    sd, wave = R.base_state_dict(), R.make_wave(1, 16000, 31)
    with torch.no_grad():
        ref = R.features(sd, R.BASE, wave, 9)
    m = _model(R.BASE, sd, 9, torch.randn(500, 768, generator=_gen(1)))
    h = m.features(wave.to(dev))
    assert h.shape == (1, 49, 768)
    a = R.movement(h.cpu().double(), ref)
    print(f"BASE T 16000 layer 9: vs fp64 {a:.3e}, tolerance {tol:.3e}")
    assert a < tol
    assert torch.equal(m(wave.to(dev)), m.assign(h))


@gpu
def test_code_agreement_small():
    """at most 5 % of 198 frames carry a code other than the fp64 restatement's argmin, and every differing frame still satisfies
    the k-means contract on the device's OWN features"""
    m = _small()
    wave = R.make_wave(2, 400 + 320 * 98, 77)
    with torch.no_grad():
        ref = R.features(R.small_state_dict(), R.SMALL, wave, 4)
    c = m.cluster_centers.cpu()
    want, _ = R.kmeans_assign(ref, c)
    h, ids = m.features(wave.to(dev)), m(wave.to(dev)).cpu()
    differ = ids != want
    print(f"code agreement SMALL: {int(differ.sum())} of {differ.numel()} frames differ")
    assert differ.numel() == 198 and differ.float().mean() <= 0.05
    ok, _ = _contract_ok(h.cpu().reshape(-1, 128), c, ids.reshape(-1))
    assert ok.all()


@gpu
def test_output_layer_runs_only_its_layers():
    """output_layer = 2 of 4: layers 3 and 4 are loaded, never packed or launched -- the same bits as a 2-layer model"""
    import voicebox_pytorch_amd as vbx

    wave = R.make_wave(2, 5000, 3).to(dev)
    m4 = _small(2)
    assert len(m4._cached(m4._pack)["layers"]) == 2
    cfg2 = dict(R.SMALL, num_hidden_layers=2)
    sd2 = {k: v for k, v in R.small_state_dict().items() if not k.startswith(("encoder.layers.2.", "encoder.layers.3."))}
    m2 = _model(cfg2, sd2, 2, m4.cluster_centers.cpu())
    assert torch.equal(m4.features(wave), m2.features(wave)) and torch.equal(m4(wave), m2(wave))
    # ... and as many launches: every entry point goes through _lib.call or the module's _gemm
    from voicebox_pytorch_amd import _lib

    def launches(m):
        n, call, gemm = [0], _lib.call, type(m)._gemm
        count = lambda f: (lambda *a, **k: (n.__setitem__(0, n[0] + 1), f(*a, **k))[1])
        _lib.call, type(m)._gemm = count(call), staticmethod(count(gemm))
        try:
            m(wave)
        finally:
            _lib.call, type(m)._gemm = call, staticmethod(gemm)
        return n[0]

    n2 = launches(m2)
    assert launches(m4) == n2 == 2 + 6 + 4 + 2 * 8 + 1 and launches(_small(4)) == n2 + 2 * 8  # eight launches per layer


@gpu
def test_input_sample_hz_is_resample_then_call():
    import voicebox_pytorch_amd as vbx

    m = _small()
    wave = R.make_wave(2, 9000, 4).to(dev)
    assert torch.equal(m(wave, input_sample_hz=24000), m(vbx.resample(wave, 24000, 16000)))
    assert torch.equal(m(wave, input_sample_hz=16000), m(wave))


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
    # mark_weights_dirty after a write through .data
    wave = R.make_wave(1, 2000, 9).to(dev)
    h0 = m.features(wave)
    p = m.encoder.layers[0].attention.out_proj.bias
    old = p.data.clone()
    p.data.add_(0.5)
    m.mark_weights_dirty()
    assert not torch.equal(m.features(wave), h0)
    p.data.copy_(old)
    m.mark_weights_dirty()
    assert torch.equal(m.features(wave), h0)


@gpu
def test_code_agreement_base_widths():
    """the same cap at the base widths, layer 9, K = 500 (198 frames)"""
    sd, c = R.base_state_dict(), R.codebook("BASE", 0, 9, 500)
    m = _model(R.BASE, sd, 9, c)
    wave = R.make_wave(2, 400 + 320 * 98, 77)
    with torch.no_grad():
        want, _ = R.kmeans_assign(R.features(sd, R.BASE, wave, 9), c)
    h, ids = m.features(wave.to(dev)), m(wave.to(dev)).cpu()
    differ = ids != want
    print(f"code agreement BASE layer 9: {int(differ.sum())} of {differ.numel()} frames differ")
    assert differ.numel() == 198 and differ.float().mean() <= 0.05
    ok, _ = _contract_ok(h.cpu().reshape(-1, 768), c, ids.reshape(-1))
    assert ok.all()


# ------------------------------------------------------------------------------------ the wrapper
VB_KW = dict(dim=128, num_cond_tokens=64, depth=2, dim_head=64, heads=2, condition_on_text=True, time_hidden_dim=128, ff_mult=2)


def _wrapper(state=None, **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(audio_enc_dec=vbx.LogMelCodec(), **VB_KW)
    if state is not None:
        vb.load_state_dict(state)
    return vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev), **kw)


def _draws(shape, seed=5):
    g = _gen(seed)
    return dict(x0=torch.randn(shape, generator=g), times=torch.rand(shape[0], generator=g), frac_lengths=torch.tensor([0.8, 0.9]),
                rand=torch.rand(shape[0], generator=g))


class _StubWav2Vec:
    """any object with the two rates and forward(wave) -> ids serves as wav2vec"""
    target_sample_hz, downsample_factor = 16000, 320

    def __init__(self, ids):
        self.ids, self.seen = ids, None

    def __call__(self, wave):
        self.seen = tuple(wave.shape)
        return self.ids


@gpu
def test_wrapper_computes_semantic_ids_from_the_wave():
    """wrapper(wave) with wav2vec=tok is wrapper(wave, semantic_token_ids=tok(resample(wave, 24000, 16000))) bit for bit, for forward
    and for TrainStep.step; given ids are used as before; latents without ids keep asserting; a stub serves; text_to_semantic raises"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override

    torch.manual_seed(3)
    tok = _small()
    w_tok = _wrapper(wav2vec=tok)
    start = {k: v.detach().cpu().clone() for k, v in w_tok.voicebox.state_dict().items()}
    w_ids = _wrapper(state=start)
    wave = R.make_wave(2, 9600, 8, rate=24000).to(dev)  # 24 kHz, LogMelCodec's rate: 61 latent frames, 19 semantic frames
    ids = tok(vbx.resample(wave, 24000, 16000))
    assert ids.shape == (2, 19) and len(ids.unique()) > 4
    draws = _draws((2, 61, 100))
    with rng_override(**draws):
        a = w_tok(wave)
    with rng_override(**draws):
        b = w_ids(wave, semantic_token_ids=ids)
    with rng_override(**draws):
        c = w_tok(wave, semantic_token_ids=ids)  # given ids are used as before
    assert torch.isfinite(a) and torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), c.detach())
    other = ids.flip(1).contiguous()
    with rng_override(**draws):
        e = w_ids(wave, semantic_token_ids=other)
    assert not torch.equal(e.detach(), a.detach())  # the ids matter
    stub = _StubWav2Vec(other)
    w_stub = _wrapper(state=start, wav2vec=stub)
    with rng_override(**draws):
        f = w_stub(wave)
    assert torch.equal(f.detach(), e.detach()) and stub.seen == (2, 6400)
    lat = w_ids.voicebox.audio_enc_dec.encode(wave)
    with pytest.raises(AssertionError):
        w_tok(lat)  # latents without ids: nothing to make ids from
    with pytest.raises(AssertionError):
        w_ids(wave)  # no wav2vec: as before
    with pytest.raises(NotImplementedError, match="TextToSemantic"):
        _wrapper(text_to_semantic=object())
    with rng_override(**draws):
        l1 = TrainStep(w_tok, lr=1e-3, max_grad_norm=0.5).step(wave)
    with rng_override(**draws):
        l2 = TrainStep(w_ids, lr=1e-3, max_grad_norm=0.5).step(wave, cond_token_ids=ids)
    assert torch.isfinite(l1) and torch.equal(l1.detach(), l2.detach())
    sd1, sd2 = w_tok.voicebox.state_dict(), w_ids.voicebox.state_dict()
    # every weight after the step, bit for bit -- but the embedding table, whose gradient vbx_cond_emb_bwd sums with fp32 atomics
    differ = [k for k in sd1 if k != "to_cond_emb.weight" and not torch.equal(sd1[k], sd2[k])]
    assert not differ, differ
    assert not torch.equal(sd1["to_pred.weight"].cpu(), start["to_pred.weight"])
    assert all(torch.equal(v.cpu(), R.small_state_dict()[k]) for k, v in tok.state_dict().items() if k != "cluster_centers")  # never trained


@gpu
def test_sample_sizes_cond_by_the_wav2vec_frame_rate():
    """sample(cond=latents, semantic_token_ids=ids): ceil(n_ids * (16000 / 320) / (24000 / 160)) frames with wav2vec set (the reference's
    rule, voicebox_pytorch.py:1254-1255), n_ids frames without it"""
    import math

    torch.manual_seed(4)
    w_tok = _wrapper(wav2vec=_small())
    w_ids = _wrapper(state=w_tok.voicebox.state_dict())
    lat = torch.randn(2, 30, 100, generator=_gen(2)).to(dev)
    ids = torch.randint(0, 64, (2, 19), generator=_gen(3)).to(dev)
    want = math.ceil(19 * (16000 / 320) / (24000 / 160))
    assert want == 7
    a = w_tok.sample(cond=lat, semantic_token_ids=ids, steps=2, decode_to_audio=False)
    b = w_ids.sample(cond=lat, semantic_token_ids=ids, steps=2, decode_to_audio=False)
    assert a.shape == (2, want, 100) and b.shape == (2, 19, 100) and torch.isfinite(a).all() and torch.isfinite(b).all()
    with pytest.raises(NotImplementedError, match="TextToSemantic"):
        w_tok.sample(cond=lat, texts=["a", "b"])
