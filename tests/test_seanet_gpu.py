"""voicebox_pytorch_amd.SEANetEncoder on the device (csrc/seanet.hip) against the restatement tests/seanet_ref.py.

Single convolutions: fp64 on the same fp16-rounded operands under a DERIVED per-element bound, in the form of
tests/test_resample_gpu.py: (K + 2) * 2^-24 * sum |w x| for any fp32 summation order of K products plus the bias, 2^-11 |y| (and
half a subnormal step, 2^-25) where the output is stored as fp16, and -- with the ELU prologue on -- one fp16 ulp times |w| for
every operand whose ELU lies within 2 fp32 ulps of an fp16 rounding boundary (expm1f need not round as the host's does).
The LSTM and the whole encoder: max |delta| / RMS(reference) against the emulated-precision restatement (BOUND_A / LSTM_BOUND: only
fp32 summation order and fp16 boundary flips differ) and against plain fp64 (BOUND_B: what fp16 operands cost), each 2 x the largest
value measured on an MI355X over the listed shapes and seeds 0 .. 2 (profiles/seanet_parity.txt).  Parity with the `encodec`
library itself is UNPINNED."""
import functools

import pytest
import torch
import torch.nn.functional as F

import seanet_ref as S

gpu = pytest.mark.gpu
dev = "cuda"

# 2 x the largest measured (profiles/seanet_parity.txt).  Worst cases: BOUND_A real B 2 T 3237 seed 1 (1.407e-3);
# BOUND_B small B 2 T 1061 seed 0 (2.843e-3); LSTM_BOUND H 64 layers 2 T 9 B 3 seed 1 (7.863e-6).
BOUND_A = 2.82e-3
BOUND_B = 5.69e-3
LSTM_BOUND = 1.58e-5


def _wave(B, T, seed):
    return 0.3 * torch.randn(B, T, generator=torch.Generator().manual_seed(1000 + seed))


# ------------------------------------------------------------------------------------ single convolutions
#        name            C1   C2   Co   k  stride dil  elu  out_f32
CONVS = [("32-16 k3", 32, 0, 16, 3, 1, 1, True, False),
         ("tail 16|32-32", 16, 32, 32, 1, 1, 1, True, False),
         ("32-64 k4 s2", 32, 0, 64, 4, 2, 1, True, False),
         ("64-128 k8 s4", 64, 0, 128, 8, 4, 1, True, False),
         ("128-256 k10 s5", 128, 0, 256, 10, 5, 1, True, False),
         ("256-512 k16 s8", 256, 0, 512, 16, 8, 1, True, False),
         ("512-128 k7 f32", 512, 0, 128, 7, 1, 1, True, True),
         ("32-16 k3 d2", 32, 0, 16, 3, 1, 2, True, False),
         ("512-1024 k16 s8", 512, 0, 1024, 16, 8, 1, True, False)]  # the widest the constructor accepts (n_filters 64): 138 KiB of LDS


def _lengths(k, stride, dil, tile):
    """1; the longest L the short-input rule still serves, and that plus 1; an L that is no multiple of the stride; the L that
    gives exactly one output more than the kernel's time tile.  Rows shorter than the tile are launched with a tile clamped to
    the next power of two >= Lout (at least 16), so over these lengths every case runs its full tile once and the 16-position
    tile at least once.  Which of the kernel's three instantiations (1, 2 or 4 position blocks per work item) a launch selects
    follows from (tile / 16) and (Co / 16): at the full tile 4 for the tail, 32-64, 64-128 and 512-128, 2 for 32-16 (one channel
    block) and 128-256 (tile 32), 1 for 256-512 and 512-1024 (tile 16); every clamped 16-position launch runs 1.  So all three
    run in this test."""
    short = [L for L in range(1, (k - 1) * dil + 2 + stride) if L <= max(S.conv_pads(L, k, stride, dil)[0], sum(S.conv_pads(L, k, stride, dil)[1:]))]
    Ls = {1, 3 * stride + 1 if stride > 1 else 37, tile * stride + 1}
    if short:
        Ls |= {max(short), max(short) + 1}
    return sorted(Ls)


def _ulp16(a):
    return torch.maximum(2.0 ** (torch.floor(torch.log2(a.abs().clamp_min(2.0 ** -14))) - 10), torch.tensor(2.0 ** -24, dtype=torch.float64))


def _elu_operand(x16):
    """x fp16 -> (the operand fp16(ELU_fp32(x)) as fp64, the set where 2 fp32 ulps either way change that rounding)"""
    e = F.elu(x16.double())
    e32 = e.float()
    lo = torch.nextafter(torch.nextafter(e32, torch.full_like(e32, -float("inf"))), torch.full_like(e32, -float("inf")))
    hi = torch.nextafter(torch.nextafter(e32, torch.full_like(e32, float("inf"))), torch.full_like(e32, float("inf")))
    return e32.half().double(), lo.half() != hi.half()


@gpu
@pytest.mark.parametrize("case", CONVS, ids=[c[0] for c in CONVS])
def test_single_convolution(case):
    from voicebox_pytorch_amd import _lib

    name, C1, C2, Co, k, stride, dil, elu, out_f32 = case
    tile = _lib.call_value("vbx_seanet_conv_tile", C1, C2, k, stride, dil)
    assert tile in (16, 32, 64, 128)
    g = torch.Generator().manual_seed(len(name) + 7 * C1)
    w = (torch.randn(Co, C1, k, generator=g) / (C1 * k) ** 0.5).half()
    w2 = (torch.randn(Co, C2, 1, generator=g) / max(C2, 1) ** 0.5).half()
    bias = 0.1 * torch.randn(Co, generator=g)
    wk = torch.cat([w.permute(0, 2, 1).reshape(Co, k * C1), w2[:, :, 0]], dim=1).contiguous().to(dev)
    K = k * C1 + C2
    for L in _lengths(k, stride, dil, tile):
        B, Lout = 2, -(-L // stride)
        x = torch.randn(B, L, C1, generator=g).half()
        x[1] = 0.75  # a constant second row: a halo read across the batch boundary would show in row 0
        x2 = torch.randn(B, L, max(C2, 8), generator=g).half()
        x2[1] = -0.5
        y = torch.full((B + 1, Lout, Co), float("nan"), dtype=torch.float32 if out_f32 else torch.float16, device=dev)
        args = (x.to(dev), x2.to(dev) if C2 else None, wk, bias.to(dev), y, B, L, C1, C2, Co, k, stride, dil, int(elu), int(out_f32),
                _lib.current_stream())
        _lib.call("vbx_seanet_conv", *args)
        first = y.clone()
        _lib.call("vbx_seanet_conv", *args)
        assert torch.equal(first[:B], y[:B]), (name, L, "rerun differs")
        assert bool(torch.isnan(y[B]).all()), (name, L, "wrote past the last row")
        got = y[:B].double().cpu()
        assert bool(torch.isfinite(got).all()), (name, L)
        # fp64 on the same operands
        a, near = _elu_operand(x) if elu else (x.double(), torch.zeros_like(x, dtype=torch.bool))
        a, near = a.transpose(1, 2), near.transpose(1, 2)
        ref = S.sconv(a, w.double(), bias.double(), stride=stride, dilation=dil)
        mag = S.sconv(a.abs(), w.double().abs(), None, stride=stride, dilation=dil) + bias.double().abs()[None, :, None]
        flip = S.sconv(near.double() * _ulp16(a), w.double().abs(), None, stride=stride, dilation=dil)
        if C2:
            b2 = x2.double().transpose(1, 2)
            ref = ref + F.conv1d(b2, w2.double())
            mag = mag + F.conv1d(b2.abs(), w2.double().abs())
        ref, mag, flip = ref.transpose(1, 2), mag.transpose(1, 2), flip.transpose(1, 2)
        assert got.shape == ref.shape == (B, Lout, Co)
        bound = (K + 2) * 2.0 ** -24 * mag + flip
        if not out_f32:
            bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        err = (got - ref).abs()
        ratio = float((err / bound).max())
        print(f"seanet conv {name} L {L} (tile <= {tile}) K {K}: max |err| {float(err.max()):.3e}, max |err| / bound {ratio:.4f}, "
              f"operands near an fp16 boundary {int(near.sum())}")
        assert bool((err <= bound).all()), (name, L, ratio)


@gpu
def test_first_convolution():
    """1 -> 32, k 7, fp32 wave and weights: the same lengths, sentinel and neighbour checks"""
    from voicebox_pytorch_amd import _lib

    g = torch.Generator().manual_seed(11)
    w = torch.randn(32, 1, 7, generator=g) / 7 ** 0.5
    bias = 0.1 * torch.randn(32, generator=g)
    for L in (1, 3, 4, 37, 257):
        x = torch.randn(2, L, generator=g)
        x[1] = 0.75
        y = torch.full((3, L, 32), float("nan"), dtype=torch.float16, device=dev)
        args = (x.to(dev), w[:, 0].contiguous().to(dev), bias.to(dev), y, 2, L, 32, 7, _lib.current_stream())
        _lib.call("vbx_seanet_conv0", *args)
        first = y.clone()
        _lib.call("vbx_seanet_conv0", *args)
        assert torch.equal(first[:2], y[:2]) and bool(torch.isnan(y[2]).all())
        got = y[:2].double().cpu()
        ref = S.sconv(x.double()[:, None], w.double(), bias.double()).transpose(1, 2)
        mag = (S.sconv(x.double().abs()[:, None], w.double().abs(), None) + bias.double().abs()[None, :, None]).transpose(1, 2)
        bound = (7 + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        err = (got - ref).abs()
        print(f"seanet conv0 L {L}: max |err| {float(err.max()):.3e}, max |err| / bound {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), L


# ------------------------------------------------------------------------------------ the LSTM
def _lstm_op(sd, H, layers):
    h = lambda t: t.float().half().contiguous().to(dev)
    op = dict(H=H, layers=layers, wih0=h(sd["l.weight_ih_l0"]), whh0=h(sd["l.weight_hh_l0"]),
              b0=(sd["l.bias_ih_l0"].float() + sd["l.bias_hh_l0"].float()).to(dev), wcat1=None, b1=None)
    if layers == 2:
        op["wcat1"] = h(torch.cat([sd["l.weight_ih_l1"], sd["l.weight_hh_l1"]], dim=1))
        op["b1"] = (sd["l.bias_ih_l1"].float() + sd["l.bias_hh_l1"].float()).to(dev)
    return op


@gpu
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("H", [64, 512])
def test_lstm(H, layers):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    worst = 0.0
    for seed in (0, 1, 2):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            sd = {"l." + k: v.detach().clone() for k, v in torch.nn.LSTM(H, H, layers).state_dict().items()}
        op = _lstm_op(sd, H, layers)
        for T in (1, 2, 9):
            for B in (1, 3):
                x = torch.randn(B, T, H, generator=torch.Generator().manual_seed(seed * 100 + T * 10 + B)).half()
                ref = S.lstm(x.double(), sd, "l", layers, emulate=True) + x.double()

                def run(xx):
                    y32 = torch.full((xx.shape[0] + 1, T, H), float("nan"), device=dev)
                    y16 = vbx.SEANetEncoder.lstm_forward(op, xx.to(dev), xx.shape[0], T, _lib.current_stream(), y32=y32)
                    assert bool(torch.isnan(y32[-1]).all())
                    assert torch.equal(y16, y32[:-1].half())  # the stored activation is the fp32 result rounded once
                    return y32[:-1]

                got = run(x)
                assert torch.equal(got, run(x))  # reruns: the same bits
                for b in range(B):  # a row alone is the row inside the batch
                    assert torch.equal(run(x[b:b + 1])[0], got[b]), (H, layers, T, B, b)
                e = S.rel_err(got, ref)
                worst = max(worst, e)
                print(f"seanet lstm H {H} layers {layers} T {T} B {B} seed {seed}: max |delta| / RMS vs emulated {e:.3e}")
                assert e <= LSTM_BOUND, (H, layers, T, B, seed, e)
    print(f"seanet lstm H {H} layers {layers}: worst {worst:.3e}, LSTM_BOUND {LSTM_BOUND}")


@gpu
def test_lstm_second_batch_chunk():
    """B = 17: the step kernel's second chunk of 16 batch rows (blockIdx.z = 1); row 16 alone equals row 16 in the batch"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    H, layers, T, B = 64, 2, 3, 17
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        sd = {"l." + k: v.detach().clone() for k, v in torch.nn.LSTM(H, H, layers).state_dict().items()}
    op = _lstm_op(sd, H, layers)
    x = torch.randn(B, T, H, generator=torch.Generator().manual_seed(17)).half()
    ref = S.lstm(x.double(), sd, "l", layers, emulate=True) + x.double()

    def run(xx):
        y32 = torch.full((xx.shape[0] + 1, T, H), float("nan"), device=dev)
        vbx.SEANetEncoder.lstm_forward(op, xx.to(dev), xx.shape[0], T, _lib.current_stream(), y32=y32)
        assert bool(torch.isnan(y32[-1]).all())
        return y32[:-1]

    got = run(x)
    assert torch.equal(got, run(x)) and torch.equal(run(x[16:17])[0], got[16]) and torch.equal(run(x[:16]), got[:16])
    e = S.rel_err(got, ref)
    print(f"seanet lstm H {H} layers {layers} T {T} B {B}: max |delta| / RMS vs emulated {e:.3e}")
    assert e <= LSTM_BOUND, e


# ------------------------------------------------------------------------------------ the whole encoder
SMALL_KW = dict(n_filters=16, ratios=(4, 2), dimension=32, lstm=2)
ENCODER_CASES = [("small", 2, 5), ("small", 2, 131), ("small", 2, 1061), ("real", 2, 3237), ("real", 1, 321), ("real", 1, 5)]


@functools.lru_cache(maxsize=None)
def _reference(name, B, T, seed):
    cfg = S.SMALL if name == "small" else S.config()
    sd = S.random_state(cfg, seed)
    wave = _wave(B, T, seed)
    return sd, wave, S.encode(sd, cfg, wave, emulate=True), S.encode(sd, cfg, wave)


def _encoder(name, sd):
    import voicebox_pytorch_amd as vbx

    enc = vbx.SEANetEncoder(**(SMALL_KW if name == "small" else {}))
    enc.load_state_dict(sd)
    return enc.to(dev).eval()


@gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name,B,T", ENCODER_CASES, ids=[f"{n}-B{b}-T{t}" for n, b, t in ENCODER_CASES])
def test_encoder_parity(name, B, T, seed):
    sd, wave, emu, ref = _reference(name, B, T, seed)
    enc = _encoder(name, sd)
    got = enc(wave.to(dev))
    assert got.dtype == torch.float32 and got.shape == ref.shape == (B, enc.frames(T), enc.dimension) and got.is_contiguous()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, enc(wave.to(dev)))  # reruns: the same bits
    assert torch.equal(got, enc(wave[:, None].to(dev))) and torch.equal(got, enc(wave.double().to(dev)))  # [B, 1, T]; other float dtypes
    for b in range(B):  # a row does not depend on its neighbours
        assert torch.equal(enc(wave[b:b + 1].to(dev))[0], got[b]), (name, T, b)
    a, bb = S.rel_err(got, emu), S.rel_err(got, ref)
    print(f"seanet encoder {name} B {B} T {T} seed {seed}: max |delta| / RMS vs emulated {a:.3e} (BOUND_A {BOUND_A}), "
          f"vs fp64 {bb:.3e} (BOUND_B {BOUND_B}); emulated vs fp64 {S.rel_err(emu, ref):.3e}")
    assert a <= BOUND_A, (name, B, T, seed, a)
    assert bb <= BOUND_B, (name, B, T, seed, bb)


# ------------------------------------------------------------------------------------ codec and model
def _codec(seed=0):
    import voicebox_pytorch_amd as vbx

    sd = S.random_state(S.SMALL, seed)
    enc = vbx.SEANetEncoder(**SMALL_KW)
    enc.load_state_dict(sd)
    g = torch.Generator().manual_seed(seed)
    rvq = vbx.ResidualVQ(dim=32, codebook_size=64, num_quantizers=4)
    rvq.load_state_dict({"codebooks": 0.5 ** torch.arange(4.0)[:, None, None] * torch.randn(4, 64, 32, generator=g)})
    voc = vbx.VocosDecoder(input_channels=32, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64)
    return vbx.EncodecVocoCodec(rvq=rvq, vocoder=voc, encoder=enc, downsample_factor=enc.hop_length).to(dev).eval(), enc


@gpu
def test_codec_encode_and_model_from_waves():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    codec, enc = _codec()
    wave = _wave(2, 190, 0).to(dev)
    frames = enc.frames(190)
    assert frames == 24
    lat = codec.encode(wave)
    assert lat.shape == (2, frames, 32) and lat.dtype == torch.float32
    assert torch.equal(lat, codec.codes_to_latents(codec.decode_to_codes(enc(wave))))
    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=64, depth=2, heads=2, audio_enc_dec=codec, condition_on_text=False).to(dev)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    g = torch.Generator().manual_seed(5)
    draws = dict(x0=torch.randn(2, frames, 32, generator=g), times=torch.rand(2, generator=g), frac_lengths=torch.tensor([0.8, 0.9]),
                 rand=torch.rand(2, generator=g))
    with rng_override(**draws):
        a = wrapper(wave)
        b = wrapper(codec.encode(wave))
    assert bool(torch.isfinite(a)) and torch.equal(a.detach(), b.detach())
    y0 = torch.randn(2, frames, 32, generator=g)
    with rng_override(y0=y0):
        codes = wrapper.sample(cond=wave, steps=2, decode_to_codes=True)
    assert codes.dtype == torch.int64 and codes.shape == (2, 4, frames)


@gpu
def test_weights_repack_on_version_bump_or_mark_dirty():
    codec, enc = _codec(seed=1)
    wave = _wave(2, 190, 1).to(dev)
    base = enc(wave)
    p = enc.model[1].shortcut.conv.conv.weight_g
    p.data.mul_(2)  # through .data: neither the version counter nor the storage moves
    assert torch.equal(enc(wave), base)
    enc.mark_weights_dirty()
    doubled = enc(wave)
    assert not torch.equal(doubled, base)
    with torch.no_grad():
        p.mul_(0.5)  # in place: the version counter moves, the operands are packed again
    assert torch.equal(enc(wave), base)
