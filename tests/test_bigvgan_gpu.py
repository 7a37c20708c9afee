"""voicebox_pytorch_amd.BigVGANGenerator on the device (csrc/bigvgan.hip) against the restatement tests/bigvgan_ref.py.

Single kernels, at row lengths shorter than Activation1d's reach of +-6 and on both sides of every tile; the last batch row is
constant (a halo read across the batch boundary would show in the row before), outputs are NaN-filled one row too long (nothing
past the last row may be written, everything inside must be), every call runs twice and must return the same bits:
  vbx_bigvgan_act     fp64 on the SAME fp16 inputs and fp32 parameters under the per-element bound derived in include/vbx.h
                      (bigvgan_ref.act_bound): 7 eps 2 sum |f_u x| for the six-term sum; that and the argument's rounding eps |alpha u|
                      through |ds/du| <= 1 + alpha inv_beta, sinf within 4 ulp (the OpenCL C figure, ASSUMED), the square's and the
                      fmaf's roundings; 13 eps sum |f_d s| for the twelve-term sum; the fp16 store 2^-11 |y| + 2^-25
  vbx_bigvgan_conv    torch.equal with vbx_bigvgan_act + vbx_hifigan_conv(act = 0)
  vbx_bigvgan_convtr  torch.equal with vbx_hifigan_convtr(slope = 1.0) up to 1024 channels; at 1536 inside vbx_hifigan_convtr's bound
                      (2 C + 2) 2^-24 (sum |w a| + |b|) + 2^-11 |y| + 2^-25
  vbx_bigvgan_post    torch.equal with vbx_bigvgan_act + vbx_hifigan_post(inputs = 1, slope = 1.0) where that is defined (a bias, tanh);
                      the clamp / no-bias form against fp64 on the act kernel's own output under (k C + 2) 2^-24 (sum |w a| + |b|):
                      vbx_hifigan_post's bound without the tanhf term
The whole generator: max |delta| / RMS(reference) against the emulated-precision restatement and against plain fp64, both inside
bigvgan_tol.parity_tolerance() -- a tenth of the smallest whole-network planted fault's movement, measured in
tests/test_bigvgan_cpu.py; measured values go to profiles/bigvgan_parity.txt.  Parity with the BigVGAN library is UNPINNED."""
import functools

import pytest
import torch

import bigvgan_ref as R
import bigvgan_tol as T

gpu = pytest.mark.gpu
dev = "cuda"

LENGTHS = (1, 2, 5, 6, 7, 15, 16, 17, 63, 64, 65, 129, 257)
KD = [(3, 1), (7, 3), (11, 5), (7, 12), (11, 12)]
_measured = {}


def _record(key, line):
    _measured[key] = line
    T.write_section("gpu", [_measured[k] for k in sorted(_measured, key=str)])


def _rows(g, B, L, C, scale=1.0):
    x = (scale * torch.randn(B, L, C, generator=g)).half()
    x[B - 1] = 0.75  # a constant last row
    return x


def _mean32(xs):
    """what the kernels read from fp16 tensors xs: ((x0 + x1) + x2) / n in fp32"""
    s = xs[0].float()
    for t in xs[1:]:
        s = s + t.float()
    return s / len(xs) if len(xs) > 1 else s


def _snake(g, C, beta, alpha_hi=4.0):
    """(alpha, inv_beta) fp32 [C] as the module packs them"""
    alpha = 1.0 + (alpha_hi - 1.0) * torch.rand(C, generator=g)
    b = (1.0 + 2.0 * torch.rand(C, generator=g)) if beta else alpha
    return alpha, 1.0 / (b + 1e-9)


def _filters(g=None):
    """the published filter, or (g given) arbitrary taps: a kernel must use the buffers it is handed"""
    if g is None:
        f = R.kaiser_sinc_filter(torch.float32)
        return f, f.clone()
    return 0.3 * torch.randn(12, generator=g), 0.3 * torch.randn(12, generator=g)


def _twice(name, y, B, *args):
    """run entry point `name` (its output y NaN-filled with B + 1 rows) twice"""
    from voicebox_pytorch_amd import _lib

    _lib.call(name, *args)
    first = y.clone()
    _lib.call(name, *args)
    assert torch.equal(first[:B], y[:B]), f"{name}: rerun differs"
    assert bool(torch.isnan(y[B]).all()), f"{name}: wrote past the last row"
    assert bool(torch.isfinite(y[:B]).all()), f"{name}: an output element was not written"
    return y[:B]


def _launch_act(xs, alpha, inv_beta, f_u, f_d):
    from voicebox_pytorch_amd import _lib

    B, L, C = xs[0].shape
    y = torch.full((B + 1, L, C), float("nan"), dtype=torch.float16, device=dev)
    ptrs = [t.to(dev) for t in xs] + [None] * (3 - len(xs))
    return _twice("vbx_bigvgan_act", y, B, *ptrs, len(xs), alpha.to(dev), inv_beta.to(dev), f_u.to(dev), f_d.to(dev), y, B, L, C,
                  _lib.current_stream())


def _pack_w(w):
    """fp16 [Co, C, k] -> [Co, k * C], column tap * C + c"""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous().to(dev)


# ------------------------------------------------------------------------------------ the activation
@gpu
@pytest.mark.parametrize("beta", [True, False], ids=["snakebeta", "snake"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 24, 32, 256])
def test_activation(C, n, beta):
    g = torch.Generator().manual_seed(1000 * C + 10 * n + beta)
    worst, reach = 0.0, 0.0
    for li, L in enumerate(LENGTHS):
        xs = [_rows(g, 2, L, C, scale=1.5) for _ in range(n)]
        alpha, inv_beta = _snake(g, C, beta, alpha_hi=16.0)  # |alpha u| up to about 50
        f_u, f_d = _filters(g if li % 3 == 2 else None)
        got = _launch_act(xs, alpha, inv_beta, f_u, f_d).double().cpu().transpose(1, 2)
        x = _mean32(xs).double().transpose(1, 2)
        ref, bound = R.act_bound(x, alpha, inv_beta, f_u, f_d)
        err = (got - ref).abs()
        worst = max(worst, float((err / bound).max()))
        reach = max(reach, float((alpha.double().reshape(1, C, 1) * R.activation1d_parts(x, alpha, inv_beta, f_u, f_d)[1]).abs().max()))
        assert got.shape == ref.shape and bool((err <= bound).all()), (C, n, beta, L, float((err / bound).max()))
    print(f"bigvgan act C {C}, {n} inputs, {'snakebeta' if beta else 'snake'}: max |err| / bound {worst:.4f} over L {LENGTHS}; max |alpha u| {reach:.1f}")
    assert reach > 30.0


@gpu
def test_activation_at_the_widest_and_in_long_rows():
    """1536 channels (the limit), and a row long enough for runs of 32 positions with a partial last run"""
    from voicebox_pytorch_amd import _lib

    g = torch.Generator().manual_seed(5)
    for C, L in ((1536, 9), (16, 4099)):
        xs = [_rows(g, 2, L, C)]
        alpha, inv_beta = _snake(g, C, True)
        f_u, f_d = _filters()
        got = _launch_act(xs, alpha, inv_beta, f_u, f_d).double().cpu().transpose(1, 2)
        ref, bound = R.act_bound(xs[0].double().transpose(1, 2), alpha, inv_beta, f_u, f_d)
        assert bool(((got - ref).abs() <= bound).all()), (C, L)
    y = torch.zeros(1, 4, 1544, dtype=torch.float16, device=dev)
    with pytest.raises(_lib.VbxError):
        _lib.call("vbx_bigvgan_act", y, None, None, 1, y, y, y, y, y, 1, 4, 1544, _lib.current_stream())
    with pytest.raises(_lib.VbxError):
        _lib.call("vbx_bigvgan_act", y, None, None, 1, y, y, y, y, y, 1, 4, 12, _lib.current_stream())


# ------------------------------------------------------------------------------------ the fused convolution
@gpu
@pytest.mark.parametrize("k,d", KD, ids=[f"k{k}d{d}" for k, d in KD])
@pytest.mark.parametrize("C", [8, 24, 32, 64, 256])
def test_fused_convolution_is_activation_then_convolution(C, k, d):
    """bit-equal; a span position outside [0, L) is the convolution's ZERO padding, while A evaluated past the row would be the
    clamped (nonzero) row end: rows shorter than the halo show the difference"""
    from voicebox_pytorch_amd import _lib

    assert _lib.call_value("vbx_bigvgan_conv_tile", C, k, d) == _lib.call_value("vbx_hifigan_conv_tile", C, k, d)
    g = torch.Generator().manual_seed(3000 * C + 10 * k + d)
    w = (torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5).half()
    bias = (0.3 * torch.randn(C, generator=g)).to(dev)
    wp, st = _pack_w(w), _lib.current_stream()
    for li, L in enumerate(LENGTHS):
        x = _rows(g, 2, L, C, scale=1.5)
        alpha, inv_beta = (t.to(dev) for t in _snake(g, C, True))
        f_u, f_d = (t.to(dev) for t in _filters(g if li % 3 == 2 else None))
        h = _launch_act([x], alpha, inv_beta, f_u, f_d).contiguous()
        for res in (None, _rows(g, 2, L, C).to(dev)):
            two = torch.full((3, L, C), float("nan"), dtype=torch.float16, device=dev)
            _lib.call("vbx_hifigan_conv", h, wp, bias, res, two, 2, L, C, C, k, d, 0, 1.0, st)
            y = torch.full((3, L, C), float("nan"), dtype=torch.float16, device=dev)
            got = _twice("vbx_bigvgan_conv", y, 2, x.to(dev), alpha, inv_beta, f_u, f_d, wp, bias, res, y, 2, L, C, C, k, d, st)
            assert torch.equal(got, two[:2]), (C, k, d, L, res is not None, float((got.float() - two[:2].float()).abs().max()))


@gpu
def test_fused_convolution_refuses_what_the_convolution_refuses():
    from voicebox_pytorch_amd import _lib

    y = torch.zeros(1, 4, 1032, dtype=torch.float16, device=dev)
    f = torch.zeros(1032, device=dev)
    for C, k, d in ((1032, 3, 1), (12, 3, 1), (8, 4, 1), (8, 13, 1), (8, 3, 13), (8, 3, 0)):
        with pytest.raises(_lib.VbxError):
            _lib.call("vbx_bigvgan_conv", y, f, f, f, f, y, f, None, y, 1, 4, C, 8, k, d, _lib.current_stream())
        with pytest.raises(_lib.VbxError):
            _lib.call_value("vbx_bigvgan_conv_tile", C, k, d)


# ------------------------------------------------------------------------------------ the transposed convolution
def _launch_convtr(name, xs, wp, bias, r, *slope):
    from voicebox_pytorch_amd import _lib

    B, L, C = xs[0].shape
    y = torch.full((B + 1, L * r, C // 2), float("nan"), dtype=torch.float16, device=dev)
    ptrs = [t.to(dev) for t in xs] + [None] * (3 - len(xs))
    return _twice(name, y, B, *ptrs, len(xs), wp, bias.to(dev), y, B, L, C, r, *slope, _lib.current_stream())


@gpu
@pytest.mark.parametrize("C,r", [(16, 2), (48, 2), (256, 8)], ids=lambda v: str(v))
def test_transposed_convolution_is_hifigans_at_slope_one(C, r):
    from voicebox_pytorch_amd.hifigan import pack_convtr_weight

    g = torch.Generator().manual_seed(100 * C + r)
    w = (torch.randn(C, C // 2, 2 * r, generator=g) / (2 * C) ** 0.5).half()
    bias = 0.1 * torch.randn(C // 2, generator=g)
    wp = pack_convtr_weight(w, r).contiguous().to(dev)
    for L in LENGTHS:
        for n in (1, 3):
            xs = [_rows(g, 2, L, C) for _ in range(n)]
            ours = _launch_convtr("vbx_bigvgan_convtr", xs, wp, bias, r)
            theirs = _launch_convtr("vbx_hifigan_convtr", xs, wp, bias, r, 1.0)
            assert torch.equal(ours, theirs), (C, r, L, n)


@gpu
def test_transposed_convolution_at_1536_channels():
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.hifigan import pack_convtr_weight

    C, r = 1536, 4
    g = torch.Generator().manual_seed(1536)
    w = (torch.randn(C, C // 2, 2 * r, generator=g) / (2 * C) ** 0.5).half()
    bias = 0.1 * torch.randn(C // 2, generator=g)
    wp = pack_convtr_weight(w, r).contiguous().to(dev)
    worst = 0.0
    for L, n in ((1, 1), (2, 2), (17, 3), (33, 1)):
        xs = [_rows(g, 2, L, C) for _ in range(n)]
        got = _launch_convtr("vbx_bigvgan_convtr", xs, wp, bias, r).double().cpu()
        a = _mean32(xs).half().double().transpose(1, 2)  # the mean, rounded to fp16 once, not activated
        ref = R.convtr(a, w.double(), bias.double(), r).transpose(1, 2)
        mag = R.convtr(a.abs(), w.double().abs(), bias.double().abs(), r).transpose(1, 2)
        bound = (2 * C + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        err = (got - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert got.shape == ref.shape == (2, L * r, C // 2) and bool((err <= bound).all()), (L, n, float((err / bound).max()))
    print(f"bigvgan convtr 1536-768 r 4: max |err| / bound {worst:.4f}")
    # above 1536 it refuses, and vbx_hifigan_convtr still refuses 1536
    x = torch.zeros(1, 2, 1552, dtype=torch.float16, device=dev)
    y = torch.zeros(1, 8, 776, dtype=torch.float16, device=dev)
    b = torch.zeros(776, device=dev)
    big = torch.zeros(4 * 776, 2 * 1552, dtype=torch.float16, device=dev)
    with pytest.raises(_lib.VbxError):
        _lib.call("vbx_bigvgan_convtr", x, None, None, 1, big, b, y, 1, 2, 1552, 4, _lib.current_stream())
    with pytest.raises(_lib.VbxError):
        _lib.call("vbx_hifigan_convtr", x, None, None, 1, wp, b, y, 1, 2, 1536, 4, 1.0, _lib.current_stream())


# ------------------------------------------------------------------------------------ the last convolution
@gpu
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 24, 32])
def test_last_convolution(C, n):
    from voicebox_pytorch_amd import _lib

    k, st = 7, _lib.current_stream()
    g = torch.Generator().manual_seed(10 * C + n)
    w = torch.randn(1, C, k, generator=g) * 2.0 * (2.0 / (C * k)) ** 0.5  # the sum reaches beyond +-1
    bias = 0.1 * torch.randn(1, generator=g)
    wk, worst, beyond = w[0].t().contiguous().to(dev), 0.0, 0.0  # fp32 [k, C]
    for li, L in enumerate(LENGTHS + (1025,)):
        xs = [_rows(g, 2, L, C, scale=1.5) for _ in range(n)]
        alpha, inv_beta = (t.to(dev) for t in _snake(g, C, True))
        f_u, f_d = (t.to(dev) for t in _filters(g if li % 3 == 2 else None))
        ptrs = [t.to(dev) for t in xs] + [None] * (3 - n)
        h = _launch_act(xs, alpha.cpu(), inv_beta.cpu(), f_u.cpu(), f_d.cpu()).contiguous()  # fp16(A(mean)), the act kernel's own output
        # with a bias and tanh: the two launches it replaces
        two = torch.full((3, L), float("nan"), dtype=torch.float32, device=dev)
        _lib.call("vbx_hifigan_post", h, None, None, 1, wk, bias.to(dev), two, 2, L, C, k, 1.0, st)
        y = torch.full((3, L), float("nan"), dtype=torch.float32, device=dev)
        got = _twice("vbx_bigvgan_post", y, 2, *ptrs, n, alpha, inv_beta, f_u, f_d, wk, bias.to(dev), y, 2, L, C, k, 0, st)
        assert torch.equal(got, two[:2]), (C, n, L, float((got - two[:2]).abs().max()))
        # clamp, no bias: fp64 on the act kernel's output
        y = torch.full((3, L), float("nan"), dtype=torch.float32, device=dev)
        got = _twice("vbx_bigvgan_post", y, 2, *ptrs, n, alpha, inv_beta, f_u, f_d, wk, None, y, 2, L, C, k, 1, st).double().cpu()
        a = h.double().cpu().transpose(1, 2)
        pre = R.conv(a, w.double(), None)[:, 0]
        ref = torch.clamp(pre, -1.0, 1.0)
        mag = R.conv(a.abs(), w.double().abs(), None)[:, 0]
        bound = (k * C + 2) * 2.0 ** -24 * mag
        err = (got - ref).abs()
        worst, beyond = max(worst, float((err / bound.clamp(min=1e-30)).max())), max(beyond, float(pre.abs().max()))
        assert got.shape == ref.shape and bool((err <= bound).all()), (C, n, L, float((err / bound).max()))
        assert float(got.abs().max()) <= 1.0
    print(f"bigvgan post C {C}, {n} inputs: bit-equal with act + hifigan post; clamp / no bias max |err| / bound {worst:.4f}, max |argument| {beyond:.2f}")
    assert beyond > 1.0
    with pytest.raises(_lib.VbxError):
        _lib.call("vbx_bigvgan_post", h, None, None, 1, alpha, inv_beta, f_u, f_d, wk, None, y, 2, L, C, k, 2, st)


# ------------------------------------------------------------------------------------ the whole generator
CASES = [(name, 2, f) for name in ("SMALL", "SMALL2") for f in (1, 2, 17, 70)] + [("WIDE", 1, 3)]


@functools.lru_cache(maxsize=None)
def _reference(name, B, frames, log=False):
    cfg = getattr(R, name)
    sd = R.random_state(cfg, 0)
    mel = R.mels(B, cfg["n_mels"], frames, frames, amplitude=log)
    return sd, mel, R.generate(sd, cfg, mel, emulate=True, input_log=log), R.generate(sd, cfg, mel, input_log=log)


def _generator(name, sd, **kw):
    import voicebox_pytorch_amd as vbx

    gen = vbx.BigVGANGenerator(**getattr(R, name), **kw)
    gen.load_state_dict(sd, strict=True)
    return gen.to(dev).eval()


@gpu
@pytest.mark.parametrize("name,B,frames", CASES, ids=[f"{n}-B{b}-F{f}" for n, b, f in CASES])
def test_generator_parity(name, B, frames):
    tol = T.parity_tolerance()[0]
    sd, mel, emu, ref = _reference(name, B, frames)
    gen = _generator(name, sd)
    default = gen.fuse_act_max_channels
    got = gen(mel.to(dev))
    assert got.dtype == torch.float32 and got.shape == ref.shape == (B, frames * gen.hop_length) and got.is_contiguous()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
    assert torch.equal(got, gen(mel.to(dev)))  # reruns: the same bits
    assert torch.equal(got, gen(mel.double().to(dev)))  # other float dtypes
    assert torch.equal(got, gen(mel.half().to(dev)))  # the pack rounds to fp16 once: rounding before it changes nothing
    for fuse in (0, None, default):  # fused nowhere, everywhere, the default: the same bits
        gen.fuse_act_max_channels = fuse
        assert torch.equal(got, gen(mel.to(dev))), fuse
    a, b = R.rel_err(got, emu), R.rel_err(got, ref)
    line = (f"generator {name:<6} B {B} frames {frames:>2}: max |delta| / RMS vs emulated {a:.3e}, vs fp64 {b:.3e} "
            f"(tolerance {tol:.3e}); emulated vs fp64 {R.rel_err(emu, ref):.3e}; output RMS {float(ref.pow(2).mean().sqrt()):.3f}")
    print(line)
    _record((name, frames), line)
    assert a <= tol, (name, frames, a)
    assert b <= tol, (name, frames, b)


@gpu
@pytest.mark.parametrize("name,frames", [("SMALL", 70), ("SMALL2", 17)])
def test_a_row_alone_is_the_row_in_the_batch(name, frames):
    sd, mel, _, _ = _reference(name, 2, frames)
    gen = _generator(name, sd)
    got = gen(mel.to(dev))
    for b in range(2):
        assert torch.equal(gen(mel[b:b + 1].to(dev))[0], got[b]), (name, frames, b)


@gpu
def test_operands_repack_on_version_bump_or_mark_dirty():
    sd, mel, _, _ = _reference("SMALL", 2, 17)
    gen = _generator("SMALL", sd)
    md = mel.to(dev)
    base = gen(md)
    for p in (gen.ups[1][0].weight_g, gen.resblocks[0].activations[1].act.alpha, gen.activation_post.act.beta):
        p.data.mul_(1.5)  # through .data: neither the version counter nor the storage moves
        assert torch.equal(gen(md), base)
        gen.mark_weights_dirty()
        assert not torch.equal(gen(md), base)
        with torch.no_grad():
            p.copy_(sd_value(sd, gen, p))  # in place: the version counter moves, the operands are packed again
        assert torch.equal(gen(md), base)
    with torch.no_grad():  # the filters are buffers: a new one is used as well
        gen.activation_post.downsample.lowpass.filter.mul_(0.5)
    assert not torch.equal(gen(md), base)


def sd_value(sd, gen, p):
    """the loaded value of parameter p"""
    name = next(n for n, q in gen.named_parameters() if q is p)
    return sd[name].to(p.device)


@gpu
def test_vocoder_of_logmelcodec_and_cpu_tensors():
    import voicebox_pytorch_amd as vbx

    cfg = dict(R.SMALL, n_mels=100)
    gen = vbx.BigVGANGenerator(**cfg, input_log=True)
    sd = R.random_state(cfg, 4)
    gen.load_state_dict(sd)
    codec = vbx.LogMelCodec(vocoder=gen.to(dev).eval())
    latents = (10.0 * torch.randn(2, 23, 100, generator=torch.Generator().manual_seed(0)) - 20.0).to(dev)
    wave = codec.decode(latents)
    assert wave.shape == (2, 23 * gen.hop_length) and wave.dtype == torch.float32 and bool(torch.isfinite(wave).all())
    mel = torch.pow(10.0, 0.05 * latents).transpose(1, 2)
    assert torch.equal(wave, gen(mel))
    ref = R.generate(sd, cfg, mel.cpu(), emulate=True, input_log=True)  # the logarithm in front, against the restatement
    assert R.rel_err(wave, ref) <= T.parity_tolerance()[0]
    cpu = vbx.BigVGANGenerator(**R.SMALL2)
    with pytest.raises(vbx._lib.VbxError):
        cpu(torch.zeros(1, 20, 4))
    assert cpu.conv_pre.bias.device.type == "cpu"  # a refused call moved nothing
    with pytest.raises(vbx._lib.VbxError):
        gen(torch.zeros(1, 100, 4))
    assert gen.conv_pre.bias.device.type == "cuda"
