"""voicebox_pytorch_amd.HiFiGANGenerator on the device (csrc/hifigan.hip) against the restatement tests/hifigan_ref.py.

Single kernels: fp64 on the SAME operands (teacher-forced) under the per-element bounds derived in include/vbx.h.  The staged operand
-- the fp32 leaky ReLU of the stored fp16 value, or of the fp32 mean ((x0 + x1) + x2) / n of up to three of them -- is a chain of
single correctly rounded fp32 operations and is reproduced exactly on the host, so the bounds carry no term for it:
  vbx_hifigan_conv    (k C + 3) 2^-24 (sum |w a| + |b| + |res|) + 2^-11 |y| + 2^-25   k C products + bias + residual in any fp32 order
                      (k C + 1 additions, 2 for slack), then the fp16 store
  vbx_hifigan_convtr  (2 C + 2) 2^-24 (sum |w a| + |b|) + 2^-11 |y| + 2^-25           2 C products + bias
  vbx_hifigan_post    (k C + 2) 2^-24 (sum |w a| + |b|) + 2^-22                        the fp32 chain through the 1-Lipschitz tanh, then
                      tanhf within 4 fp32 ulps of a value of at most 1; no fp16 store
  vbx_hifigan_pack    exact without the log; with it 2^-11 |y| (the store) + 2^-22 |y| + 2^-23 (logf within 4 fp32 ulps; 2^-23 absolute
                      covers a logarithm near zero, where the fp16 store's own half ulp is at most that small)
  vbx_hifigan_respair torch.equal with the two vbx_hifigan_conv launches it replaces
Shapes: L on both sides of every tile size (16, 32, 64, 128; the fused pair's 16, 48, 112) and shorter than the padding; C from one
8-channel group to 256; kernels and dilations up to the limits (11, 12).
The whole generator: max |delta| / RMS(reference) against the emulated-precision restatement and against plain fp64, both inside the
tolerance hifigan_tol.parity_tolerance() -- a tenth of the smallest planted fault's movement, measured in tests/test_hifigan_cpu.py;
measured values go to profiles/hifigan_parity.txt.  Parity with the HiFi-GAN library itself is UNPINNED."""
import functools

import pytest
import torch
import torch.nn.functional as F

import hifigan_ref as H
import hifigan_tol as T

gpu = pytest.mark.gpu
dev = "cuda"

LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 257)
KD = [(3, 1), (7, 3), (11, 5), (7, 12), (11, 12)]
SLOPE = 0.1
_measured = {}


def _record(key, line):
    _measured[key] = line
    T.write_section("gpu", [_measured[k] for k in sorted(_measured)])


def _rows(g, B, L, C, scale=1.0):
    x = (scale * torch.randn(B, L, C, generator=g)).half()
    x[B - 1] = 0.75  # a constant last row: a halo read across the batch boundary would show in the row before
    return x


def _operand(xs, slope, round16=True):
    """what the kernels stage from fp16 tensors xs: lrelu(((x0 + x1) + x2) / n) in fp32, rounded to fp16 for an MFMA operand"""
    s = xs[0].float()
    for t in xs[1:]:
        s = s + t.float()
    if len(xs) > 1:
        s = s / len(xs)
    a = F.leaky_relu(s, slope)
    return (a.half() if round16 else a).double()


def _conv_ref(x, w, bias, res, k, d, act):
    """x fp16 [B, L, C], w fp16 [Co, C, k] -> (ref, magnitude) fp64 [B, L, Co]"""
    a = (_operand([x], SLOPE) if act else x.double()).transpose(1, 2)
    ref = H.conv(a, w.double(), bias.double(), dilation=d).transpose(1, 2)
    mag = H.conv(a.abs(), w.double().abs(), bias.double().abs(), dilation=d).transpose(1, 2)
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    return ref, mag


def _launch_conv(x, wp, bias, res, Co, k, d, act):
    from voicebox_pytorch_amd import _lib

    B, L, C = x.shape
    y = torch.full((B + 1, L, Co), float("nan"), dtype=torch.float16, device=dev)
    args = (x.to(dev), wp, bias.to(dev), None if res is None else res.to(dev), y, B, L, C, Co, k, d, int(act), SLOPE, _lib.current_stream())
    _lib.call("vbx_hifigan_conv", *args)
    first = y.clone()
    _lib.call("vbx_hifigan_conv", *args)
    assert torch.equal(first[:B], y[:B]), "rerun differs"
    assert bool(torch.isnan(y[B]).all()), "wrote past the last row"
    assert bool(torch.isfinite(y[:B]).all()), "an output element was not written"
    return y[:B]


def _pack_w(w):
    """fp16 [Co, C, k] -> [Co, k * C], column tap * C + c"""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous().to(dev)


# ------------------------------------------------------------------------------------ the convolution
@gpu
@pytest.mark.parametrize("k,d", KD, ids=[f"k{k}d{d}" for k, d in KD])
@pytest.mark.parametrize("C", [8, 16, 32, 256])
def test_single_convolution(C, k, d):
    from voicebox_pytorch_amd import _lib

    tile = _lib.call_value("vbx_hifigan_conv_tile", C, k, d)
    assert tile in (16, 32, 64, 128)
    g = torch.Generator().manual_seed(1000 * C + 10 * k + d)
    w = (torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5).half()
    bias = 0.1 * torch.randn(C, generator=g)
    wp, worst = _pack_w(w), 0.0
    for L in LENGTHS:
        x = _rows(g, 2, L, C)
        for res in (None, _rows(g, 2, L, C)):
            got = _launch_conv(x, wp, bias, res, C, k, d, True).double().cpu()
            ref, mag = _conv_ref(x, w, bias, res, k, d, True)
            bound = (k * C + 3) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25
            err = (got - ref).abs()
            worst = max(worst, float((err / bound).max()))
            assert got.shape == ref.shape and bool((err <= bound).all()), (C, k, d, L, res is not None, float((err / bound).max()))
    print(f"hifigan conv C {C} k {k} d {d} (tile <= {tile}): max |err| / bound {worst:.4f} over L {LENGTHS}, with and without res")


@gpu
def test_convolution_without_activation_and_other_widths():
    """conv_pre's form: no activation, C = 104 (100 mels padded), Co = 24 (not a multiple of 16: a column block with a tail)"""
    g = torch.Generator().manual_seed(7)
    C, Co, k = 104, 24, 7
    w = (torch.randn(Co, C, k, generator=g) / (C * k) ** 0.5).half()
    bias = 0.1 * torch.randn(Co, generator=g)
    for L in (1, 3, 65):
        x = _rows(g, 2, L, C)
        got = _launch_conv(x, _pack_w(w), bias, None, Co, k, 1, False).double().cpu()
        ref, mag = _conv_ref(x, w, bias, None, k, 1, False)
        bound = (k * C + 3) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        assert bool(((got - ref).abs() <= bound).all()), L


# ------------------------------------------------------------------------------------ the fused residual pair
@gpu
@pytest.mark.parametrize("k,d", KD, ids=[f"k{k}d{d}" for k, d in KD])
@pytest.mark.parametrize("C", [8, 32, 64])
def test_fused_pair_is_the_two_launches(C, k, d):
    """bit-equal; rows shorter than the halo make the trap visible: an intermediate position outside [0, L) is c2's ZERO padding, while
    c1 evaluated there is at least its (nonzero) bias"""
    from voicebox_pytorch_amd import _lib

    assert _lib.call_value("vbx_hifigan_respair_max_channels") == 64
    g = torch.Generator().manual_seed(2000 * C + 10 * k + d)
    w1, w2 = ((torch.randn(C, C, k, generator=g) * (2.0 / (C * k)) ** 0.5).half() for _ in range(2))
    b1, b2 = (0.3 * torch.randn(C, generator=g) for _ in range(2))
    for L in LENGTHS:
        x = _rows(g, 2, L, C)
        h = _launch_conv(x, _pack_w(w1), b1, None, C, k, d, True)
        two = _launch_conv(h.cpu(), _pack_w(w2), b2, x, C, k, 1, True)
        y = torch.full((3, L, C), float("nan"), dtype=torch.float16, device=dev)
        _lib.call("vbx_hifigan_respair", x.to(dev), _pack_w(w1), b1.to(dev), _pack_w(w2), b2.to(dev), y, 2, L, C, k, d, SLOPE,
                  _lib.current_stream())
        assert bool(torch.isnan(y[2]).all()), "wrote past the last row"
        assert torch.equal(y[:2], two), (C, k, d, L, float((y[:2].float() - two.float()).abs().max()))


# ------------------------------------------------------------------------------------ the transposed convolution
CONVTRS = [(16, 2), (32, 4), (256, 8), (32, 8), (256, 2)]


@gpu
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("C,r", CONVTRS, ids=[f"{c}-{c // 2} r{r}" for c, r in CONVTRS])
def test_transposed_convolution(C, r, n):
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.hifigan import pack_convtr_weight

    Co = C // 2
    g = torch.Generator().manual_seed(100 * C + 10 * r + n)
    w = (torch.randn(C, Co, 2 * r, generator=g) / (2 * C) ** 0.5).half()
    bias = 0.1 * torch.randn(Co, generator=g)
    wp, worst = pack_convtr_weight(w, r).contiguous().to(dev), 0.0
    for L in LENGTHS:
        xs = [_rows(g, 2, L, C) for _ in range(n)]
        y = torch.full((3, L * r, Co), float("nan"), dtype=torch.float16, device=dev)
        ptrs = [t.to(dev) for t in xs] + [None] * (3 - n)
        args = (*ptrs, n, wp, bias.to(dev), y, 2, L, C, r, SLOPE, _lib.current_stream())
        _lib.call("vbx_hifigan_convtr", *args)
        first = y.clone()
        _lib.call("vbx_hifigan_convtr", *args)
        assert torch.equal(first[:2], y[:2]) and bool(torch.isnan(y[2]).all())
        got = y[:2].double().cpu()
        assert bool(torch.isfinite(got).all()), (C, r, n, L, "an output sample was not written")
        a = _operand(xs, SLOPE).transpose(1, 2)
        ref = H.convtr(a, w.double(), bias.double(), r).transpose(1, 2)
        mag = H.convtr(a.abs(), w.double().abs(), bias.double().abs(), r).transpose(1, 2)
        assert got.shape == ref.shape == (2, L * r, Co)
        bound = (2 * C + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        err = (got - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (C, r, n, L, float((err / bound).max()))
    print(f"hifigan convtr {C}-{Co} r {r}, {n} inputs: max |err| / bound {worst:.4f} over L {LENGTHS}")


# ------------------------------------------------------------------------------------ the last convolution
@gpu
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 16, 32, 256])
def test_last_convolution(C, n):
    from voicebox_pytorch_amd import _lib

    k = 7
    g = torch.Generator().manual_seed(10 * C + n)
    w = torch.randn(1, C, k, generator=g) * (2.0 / (C * k)) ** 0.5
    bias = 0.1 * torch.randn(1, generator=g)
    wk, worst = w[0].t().contiguous().to(dev), 0.0  # fp32 [k, C]
    for L in LENGTHS + (1025,):
        xs = [_rows(g, 2, L, C, scale=1.5) for _ in range(n)]
        y = torch.full((3, L), float("nan"), dtype=torch.float32, device=dev)
        ptrs = [t.to(dev) for t in xs] + [None] * (3 - n)
        args = (*ptrs, n, wk, bias.to(dev), y, 2, L, C, k, 0.01, _lib.current_stream())
        _lib.call("vbx_hifigan_post", *args)
        first = y.clone()
        _lib.call("vbx_hifigan_post", *args)
        assert torch.equal(first[:2], y[:2]) and bool(torch.isnan(y[2]).all())
        got = y[:2].double().cpu()
        assert bool(torch.isfinite(got).all())
        a = _operand(xs, 0.01, round16=False).transpose(1, 2)
        ref = torch.tanh(H.conv(a, w.double(), bias.double()))[:, 0]
        mag = H.conv(a.abs(), w.double().abs(), bias.double().abs())[:, 0]
        bound = (k * C + 2) * 2.0 ** -24 * mag + 2.0 ** -22
        err = (got - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert got.shape == ref.shape and bool((err <= bound).all()), (C, n, L, float((err / bound).max()))
    print(f"hifigan post C {C}, {n} inputs: max |err| / bound {worst:.4f}")


# ------------------------------------------------------------------------------------ the pack
@gpu
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("M", [80, 100, 1])
def test_pack(M, log):
    from voicebox_pytorch_amd import _lib

    Mp = -(-M // 8) * 8
    for B, frames in ((2, 37), (1, 1), (3, 64)):
        mel = H.mels(B, M, frames, M, amplitude=log)
        y = torch.full((B + 1, frames, Mp), float("nan"), dtype=torch.float16, device=dev)
        _lib.call("vbx_hifigan_pack", mel.to(dev), y, B, M, frames, int(log), _lib.current_stream())
        assert bool(torch.isnan(y[B]).all())
        got = y[:B].cpu()
        assert bool((got[:, :, M:] == 0).all()), "the padding columns are zeros"
        if not log:
            assert torch.equal(got[:, :, :M], mel.transpose(1, 2).half())
        else:
            ref = torch.log(torch.clamp(mel.double(), min=1e-5)).transpose(1, 2)
            err = (got[:, :, :M].double() - ref).abs()
            assert bool((err <= (2.0 ** -11 + 2.0 ** -22) * ref.abs() + 2.0 ** -23).all()), float(err.max())


# ------------------------------------------------------------------------------------ the whole generator
CASES = [(name, 2, f, False) for name in ("SMALL", "SMALL2") for f in (1, 2, 17, 70)] + [("V1", 2, 12, False), ("SMALL", 2, 17, True)]


@functools.lru_cache(maxsize=None)
def _reference(name, B, frames, log):
    cfg = getattr(H, name)
    sd = H.random_state(cfg, 0)
    mel = H.mels(B, cfg["n_mels"], frames, frames, amplitude=log)
    return sd, mel, H.generate(sd, cfg, mel, emulate=True, input_log=log), H.generate(sd, cfg, mel, input_log=log)


def _generator(name, sd, **kw):
    import voicebox_pytorch_amd as vbx

    gen = vbx.HiFiGANGenerator(**getattr(H, name), **kw)
    gen.load_state_dict(sd)
    return gen.to(dev).eval()


@gpu
@pytest.mark.parametrize("name,B,frames,log", CASES, ids=[f"{n}-B{b}-F{f}{'-log' if lg else ''}" for n, b, f, lg in CASES])
def test_generator_parity(name, B, frames, log):
    tol = T.parity_tolerance()[0]
    sd, mel, emu, ref = _reference(name, B, frames, log)
    gen = _generator(name, sd, input_log=log)
    got = gen(mel.to(dev))
    assert got.dtype == torch.float32 and got.shape == ref.shape == (B, frames * gen.hop_length) and got.is_contiguous()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
    assert torch.equal(got, gen(mel.to(dev)))  # reruns: the same bits
    assert torch.equal(got, gen(mel.double().to(dev)))  # other float dtypes
    gen.fuse_max_channels = 0  # the unfused launches: the same bits
    assert torch.equal(got, gen(mel.to(dev)))
    a, b = H.rel_err(got, emu), H.rel_err(got, ref)
    line = (f"generator {name:<6} B {B} frames {frames:>2}{' input_log' if log else ''}: max |delta| / RMS vs emulated {a:.3e}, vs fp64 {b:.3e} "
            f"(tolerance {tol:.3e}); emulated vs fp64 {H.rel_err(emu, ref):.3e}; output RMS {float(ref.pow(2).mean().sqrt()):.3f}")
    print(line)
    _record((name, frames, log), line)
    assert a <= tol, (name, frames, a)
    assert b <= tol, (name, frames, b)


@gpu
@pytest.mark.parametrize("name,frames", [("SMALL", 70), ("SMALL2", 17), ("V1", 12)])
def test_a_row_alone_is_the_row_in_the_batch(name, frames):
    sd, mel, _, _ = _reference(name, 2, frames, False)
    gen = _generator(name, sd)
    got = gen(mel.to(dev))
    for b in range(2):
        assert torch.equal(gen(mel[b:b + 1].to(dev))[0], got[b]), (name, frames, b)


@gpu
def test_weights_repack_on_version_bump_or_mark_dirty():
    sd, mel, _, _ = _reference("SMALL", 2, 17, False)
    gen = _generator("SMALL", sd)
    md = mel.to(dev)
    base = gen(md)
    p = gen.ups[1].weight_g
    p.data.mul_(2)  # through .data: neither the version counter nor the storage moves
    assert torch.equal(gen(md), base)
    gen.mark_weights_dirty()
    assert not torch.equal(gen(md), base)
    with torch.no_grad():
        p.mul_(0.5)  # in place: the version counter moves, the operands are packed again
    assert torch.equal(gen(md), base)


@gpu
def test_vocoder_of_logmelcodec_and_cpu_tensors():
    import voicebox_pytorch_amd as vbx

    cfg = dict(H.SMALL, n_mels=100)
    gen = vbx.HiFiGANGenerator(**cfg, input_log=True)
    gen.load_state_dict(H.random_state(cfg, 4))
    codec = vbx.LogMelCodec(vocoder=gen.to(dev).eval())
    latents = (10.0 * torch.randn(2, 23, 100, generator=torch.Generator().manual_seed(0)) - 20.0).to(dev)
    wave = codec.decode(latents)
    assert wave.shape == (2, 23 * gen.hop_length) and wave.dtype == torch.float32 and bool(torch.isfinite(wave).all())
    assert torch.equal(wave, gen(torch.pow(10.0, 0.05 * latents).transpose(1, 2)))
    with pytest.raises(vbx._lib.VbxError):
        gen(torch.zeros(1, 100, 4))
    assert gen.conv_pre.bias.device.type == "cuda"  # a refused call moved nothing
