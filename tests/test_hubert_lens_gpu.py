"""HubertWithKmeans(wave, lens=) on the device: the three *_lens kernels of csrc/hubert.hip and the whole network, against the PLAIN
entries on each row alone -- bit for bit on the live positions, exactly zero past them, whatever the padding holds (noise, NaN) -- and
against the fp64 restatement of the row alone inside the tolerance tests/hubert_lens_ref.tolerance_lens() MEASURES (the smaller of
hubert_ref.tolerance_small() and a tenth of the smallest planted length fault's movement; profiles/hubert_lens_parity.txt).

Bit-equality of the whole network stands on vbx_gemm_route answering the same for the batch and for the row alone: each test asserts
that first, so a later change of the routes shows up as that assertion."""
import functools

import pytest
import torch

import hubert_lens_ref as LR
import hubert_ref as R

gpu = pytest.mark.gpu
dev = "cuda"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _small(output_layer=4, seq_len_multiple_of=None):
    import voicebox_pytorch_amd as vbx

    centers = R.codebook("SMALL", 0, 4, 64)
    m = vbx.HubertWithKmeans(**R.SMALL, output_layer=output_layer, codebook_size=centers.shape[0], seq_len_multiple_of=seq_len_multiple_of)
    m.load_state_dict(R.small_state_dict())
    m.set_cluster_centers(centers)
    return m.to(dev)


# ------------------------------------------------------------------------------------ conv0 + GroupNorm under lengths
@gpu
def test_conv0_lens_is_the_row_alone():
    from voicebox_pytorch_amd import _lib

    B, C, k0, s0, eps, L0 = 4, 32, 10, 5, 1e-5, 600
    T = (L0 - 1) * s0 + k0
    l0s = [1, 255, 256, 257]
    lens = [(l - 1) * s0 + k0 + (b % 3) for b, l in enumerate(l0s)]  # up to two samples no position of the row reaches
    g = _gen(1)
    x = (3.0 + torch.randn(B, T, generator=g)).float()
    w = (torch.randn(C, k0, generator=g) * 0.3).float().to(dev)
    gam, bet = (0.75 + 0.5 * torch.rand(C, generator=g)).float().to(dev), (0.2 * torch.randn(C, generator=g)).float().to(dev)
    st = _lib.current_stream()
    chunks = _lib.call_value("vbx_hubert_conv0_chunks", L0)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)

    def run(xd):
        rec = torch.full((B, chunks, C, 3), float("nan"), device=dev)
        stats, out = torch.empty(B, C, 2, device=dev), torch.full((B, L0, C), float("nan"), dtype=torch.float16, device=dev)
        _lib.call("vbx_hubert_conv0_stats_lens", xd, ld, w, rec, stats, B, T, C, k0, s0, eps, st)
        _lib.call("vbx_hubert_conv0_apply_lens", xd, ld, w, stats, gam, bet, out, B, T, C, k0, s0, st)
        return stats.cpu(), out.cpu()

    stats, out = run(x.to(dev))
    for b, (l, l0) in enumerate(zip(lens, l0s)):
        xa = x[b:b + 1, :l].contiguous().to(dev)
        rec1 = torch.empty(1, _lib.call_value("vbx_hubert_conv0_chunks", l0), C, 3, device=dev)
        s1, o1 = torch.empty(1, C, 2, device=dev), torch.empty(1, l0, C, dtype=torch.float16, device=dev)
        _lib.call("vbx_hubert_conv0_stats", xa, w, rec1, s1, 1, l, C, k0, s0, eps, st)
        _lib.call("vbx_hubert_conv0_apply", xa, w, s1, gam, bet, o1, 1, l, C, k0, s0, st)
        assert torch.equal(stats[b], s1.cpu()[0]), (b, l0)
        assert torch.equal(out[b, :l0], o1.cpu()[0]), (b, l0)
        assert (out[b, l0:].view(torch.int16) == 0).all(), (b, l0)  # fp16 +0.0, not -0.0
    xn = x.clone()
    for b, l in enumerate(lens):
        xn[b, l:] = float("nan")
    stats_n, out_n = run(xn.to(dev))
    assert torch.equal(stats_n, stats) and torch.equal(out_n.view(torch.int16), out.view(torch.int16))
    # a full-length table is the plain entry
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    rec, s2, o2 = torch.empty(B, chunks, C, 3, device=dev), torch.empty(B, C, 2, device=dev), torch.empty(B, L0, C, dtype=torch.float16, device=dev)
    s3, o3 = torch.empty_like(s2), torch.empty_like(o2)
    _lib.call("vbx_hubert_conv0_stats", x.to(dev), w, rec, s2, B, T, C, k0, s0, eps, st)
    _lib.call("vbx_hubert_conv0_apply", x.to(dev), w, s2, gam, bet, o2, B, T, C, k0, s0, st)
    _lib.call("vbx_hubert_conv0_stats_lens", x.to(dev), full, w, rec, s3, B, T, C, k0, s0, eps, st)
    _lib.call("vbx_hubert_conv0_apply_lens", x.to(dev), full, w, s3, gam, bet, o3, B, T, C, k0, s0, st)
    assert torch.equal(s2, s3) and torch.equal(o2, o3)
    # lengths outside k0 .. T are clamped by the kernel: the ends of the range, nothing read or written out of bounds
    wild = torch.tensor([0, -7, T + 1000, 2 ** 31 - 1], dtype=torch.int32, device=dev)
    _lib.call("vbx_hubert_conv0_stats_lens", x.to(dev), wild, w, rec, s3, B, T, C, k0, s0, eps, st)
    _lib.call("vbx_hubert_conv0_apply_lens", x.to(dev), wild, w, s3, gam, bet, o3, B, T, C, k0, s0, st)
    assert torch.equal(o3[2:], o2[2:]) and (o3[:2, 1:].view(torch.int16) == 0).all() and torch.isfinite(o3).all()


# ------------------------------------------------------------------------------------ the positional convolution under lengths
@gpu
@pytest.mark.parametrize("D,G,k,N", [(128, 4, 16, None), (768, 16, 128, 40)])
def test_posconv_lens_is_the_row_alone(D, G, k, N):
    from voicebox_pytorch_amd import _lib

    tile = _lib.call_value("vbx_hubert_posconv_tile", D // G, k)
    N = N or tile + 9
    nbs = sorted({1, N} | {v for v in (15, 16, 17, tile - 1, tile, tile + 1) if 1 <= v <= N})
    B = len(nbs)
    g = _gen(D + k)
    w = (torch.randn(D, D // G, k, generator=g) * (1.0 / (k * D // G)) ** 0.5).half()
    wp = w.permute(0, 2, 1).reshape(D, -1).contiguous().to(dev)
    bias = (0.3 * torch.randn(D, generator=g)).float().to(dev)
    x = torch.randn(B, N, D, generator=g).float()
    ld = torch.tensor(nbs, dtype=torch.int32, device=dev)
    st = _lib.current_stream()

    def run(xd):
        y = torch.full((B, N, D), float("nan"), device=dev)
        _lib.call("vbx_hubert_posconv_lens", xd, ld, wp, bias, y, B, N, D, G, k, st)
        return y.cpu()

    y = run(x.to(dev))
    for b, nb in enumerate(nbs):
        y1 = torch.empty(1, nb, D, device=dev)
        _lib.call("vbx_hubert_posconv", x[b:b + 1, :nb].contiguous().to(dev), wp, bias, y1, 1, nb, D, G, k, st)
        assert torch.equal(y[b, :nb], y1.cpu()[0]), (D, nb)
        assert (y[b, nb:].view(torch.int32) == 0).all(), (D, nb)
    xn = x.clone()
    for b, nb in enumerate(nbs):
        xn[b, nb:] = float("nan")
    assert torch.equal(run(xn.to(dev)).view(torch.int32), y.view(torch.int32))
    yp = torch.empty(B, N, D, device=dev)
    _lib.call("vbx_hubert_posconv", x.to(dev), wp, bias, yp, B, N, D, G, k, st)
    _lib.call("vbx_hubert_posconv_lens", x.to(dev), torch.full((B,), N, dtype=torch.int32, device=dev), wp, bias, yf := torch.empty_like(yp), B, N, D, G, k, st)
    assert torch.equal(yp, yf)  # a full-length table is the plain entry
    wild = torch.tensor(([0, -3, N + 5, 2 ** 31 - 1] * B)[:B], dtype=torch.int32, device=dev)  # clamped into 1 .. N
    _lib.call("vbx_hubert_posconv_lens", x.to(dev), wild, wp, bias, yf, B, N, D, G, k, st)
    assert torch.isfinite(yf).all()


# ------------------------------------------------------------------------------------ the whole network
CASES = {"tiles": (41360, (41360, 20880, 20560, 400)), "odd": (5000, (5000, 3333, 1285, 719))}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(wave [4, T], lens, the fp64 restatement of each row alone): computed once, shared, never written to"""
    T, lens = CASES[name]
    wave = R.make_wave(len(lens), T, 40 + T % 89)
    with torch.no_grad():
        alone = LR.rows_alone(R.small_state_dict(), R.SMALL, wave, lens, 4)
    return wave, list(lens), alone


def _routes_equal(m, B, N, frames):
    want = m.gemm_routes(B * N)
    for f in frames:
        assert m.gemm_routes(f) == want, f"vbx_gemm_route answers differently for {B * N} rows and for {f}: no bit claim stands"


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rows_under_lens_are_the_rows_alone(name):
    m = _small()
    wave, lens, alone = _case(name)
    B, T = wave.shape
    frames = [R.frames_of(l, R.SMALL) for l in lens]
    if name == "tiles":
        assert frames == [129, 65, 64, 1]  # the attention kernel's 64-key and 128-query tile edges
    N = frames[0]
    _routes_equal(m, B, N, frames)
    assert m.frame_lens(lens) == frames and m.frame_lens(torch.tensor(lens)).tolist() == frames
    wd = wave.to(dev)
    h, ids = m.features(wd, lens=lens), m(wd, lens=lens)
    assert h.shape == (B, N, 128) and ids.shape == (B, N) and ids.dtype == torch.int64
    tol, _ = LR.tolerance_lens()
    for b, (l, f) in enumerate(zip(lens, frames)):
        one = wd[b:b + 1, :l].contiguous()
        assert torch.equal(h[b, :f], m.features(one)[0]), (name, b)
        assert torch.equal(ids[b, :f], m(one)[0]), (name, b)
        assert (h[b, f:].view(torch.int32) == 0).all() and (ids[b, f:] == 0).all(), (name, b)
        move = R.movement(h[b, :f].cpu().double(), alone[b])
        print(f"SMALL {name} row {b} len {l} ({f} frames): vs fp64 of the row alone {move:.3e}, tolerance {tol:.3e}")
        assert move < tol, (name, b, move, tol)
    # what lies behind the lengths is never read into a live frame: noise, then NaN and inf
    for fill in ("noise", "nan", "inf"):
        wn = wave.clone()
        for b, l in enumerate(lens):
            wn[b, l:] = {"noise": 5.0 * torch.randn(T - l, generator=_gen(b)), "nan": float("nan"), "inf": float("inf")}[fill]
        assert torch.equal(m.features(wn.to(dev), lens=lens).view(torch.int32), h.view(torch.int32)), (name, fill)
        assert torch.equal(m(wn.to(dev), lens=lens), ids), (name, fill)
    # the three kinds of lens
    for kind in (torch.tensor(lens), torch.tensor(lens, dtype=torch.int32), torch.tensor(lens, device=dev)):
        assert torch.equal(m.features(wd, lens=kind), h) and torch.equal(m(wd, lens=kind), ids)
    assert torch.equal(m(wd[:, None], lens=lens), ids)  # [B, 1, T]
    # a device tensor is clamped (no host look at it): past T is T, below one frame is one frame
    wild = torch.tensor([T + 99, lens[1], lens[2], 3], device=dev)
    hw = m.features(wd, lens=wild)
    assert torch.equal(hw[0], m.features(wd[:1])[0]) and torch.equal(hw[3, :1], m.features(wd[3:, :400].contiguous())[0])
    assert (hw[3, 1:] == 0).all()


@gpu
def test_full_lengths_are_the_call_without_lengths():
    m = _small()
    wave, _, _ = _case("odd")
    wd = wave.to(dev)
    full = [wave.shape[1]] * wave.shape[0]
    assert torch.equal(m.features(wd, lens=full), m.features(wd)) and torch.equal(m(wd, lens=full), m(wd))


@gpu
def test_input_sample_hz_with_lengths_is_resample_then_call():
    import voicebox_pytorch_amd as vbx

    m = _small()
    wave = R.make_wave(3, 9000, 4).to(dev)
    lens = [9000, 5001, 1234]
    lens16 = vbx.resample_lens(lens, 24000, 16000)
    want = m(vbx.resample(wave, 24000, 16000, lens=lens), lens=lens16)
    assert torch.equal(m(wave, input_sample_hz=24000, lens=lens), want)
    assert torch.equal(m(wave, input_sample_hz=24000, lens=torch.tensor(lens, device=dev)), want)
    assert torch.equal(m(wave, input_sample_hz=16000, lens=lens), m(wave, lens=lens))
    frames = m.frame_lens(lens16)
    _routes_equal(m, 3, frames[0], frames)
    one = m(wave[2:, :1234].contiguous(), input_sample_hz=24000)
    assert one.shape[1] == frames[2] and torch.equal(want[2, :frames[2]], one[0])


@gpu
def test_seq_len_multiple_of_floors_each_row():
    m, mm = _small(), _small(seq_len_multiple_of=320)
    wave, lens, _ = _case("odd")
    wd = wave.to(dev)
    floored = [l // 320 * 320 for l in lens]
    assert mm.frame_lens(lens) == m.frame_lens(floored)
    assert torch.equal(mm(wd, lens=lens), m(wd[:, :5000 // 320 * 320].contiguous(), lens=floored))
    for b, l in enumerate(lens):
        f = m.frame_lens([l // 320 * 320])[0]
        assert torch.equal(mm(wd, lens=lens)[b, :f], mm(wd[b:b + 1, :l].contiguous())[0])


@gpu
def test_refusals_under_lengths_on_the_device():
    m = _small()
    w = torch.zeros(2, 800, device=dev)
    with pytest.raises(NotImplementedError, match="mask"):
        m(w, attention_mask=torch.ones(2, 800, device=dev), lens=[800, 400])
    with pytest.raises(ValueError, match=r"HubertWithKmeans: lens\[1\] = 399 is outside 400 \.\. T = 800"):
        m(w, lens=[800, 399])
    with pytest.raises(ValueError, match="one entry per batch row"):
        m(w, lens=torch.tensor([800], device=dev))


@gpu
def test_base_widths_padded_row_is_the_unpadded_call():
    """BASE widths once: 1 x 16000 samples padded to 20000 with lens=[16000]"""
    import voicebox_pytorch_amd as vbx

    sd, wave = R.base_state_dict(), R.make_wave(1, 20000, 31)
    m = vbx.HubertWithKmeans(**R.BASE, output_layer=9, codebook_size=500)
    m.load_state_dict(sd)
    m.set_cluster_centers(torch.randn(500, 768, generator=_gen(1)))
    m = m.to(dev)
    f, N = R.frames_of(16000, R.BASE), R.frames_of(20000, R.BASE)
    _routes_equal(m, 1, N, [f])
    h = m.features(wave.to(dev), lens=[16000])
    one = m.features(wave[:, :16000].contiguous().to(dev))
    assert h.shape == (1, N, 768) and torch.equal(h[0, :f], one[0]) and (h[0, f:] == 0).all()
    ids = m(wave.to(dev), lens=[16000])
    assert torch.equal(ids[0, :f], m(wave[:, :16000].contiguous().to(dev))[0]) and (ids[0, f:] == 0).all()
