"""Training on ragged batches by lengths (lens=): the length-aware attention backward through the C ABI against the masked kernels, and
wrapper(x1, lens=) / TrainStep.step(lens=) against the mask= path and the fp64 restatement.  Under the entry points' precondition
(dout zero on the rows at or past key_lens[b]) everything is BIT-equal to the masked kernels on live rows and zero beyond; a failure of
bit-equality at model level names a kernel that reads a padding row into a live sum.  Every line that starts with PARITY is a measured
figure (profiles/train_lens_parity.txt is those lines of one run)."""
import pytest
import torch

from attn_check import rot_tables
from oracle import restate
from test_sample_lens_cpu import plant

pytestmark = pytest.mark.gpu
dev = "cuda"
Bq, H, I = 3, 2, 128
_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _st():
    return torch.cuda.current_stream().cuda_stream


def bf(x):
    return x.to(torch.bfloat16)


def key_sets(Np):
    sets = [(1, 63, 64), (65, 128, 129), (Np, Np - 1, 130)]
    return sets + [(257, 256, 17)] if Np == 272 else sets


def nans(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device=dev)


def _operands(Np):
    """fp16 operands as test_attn_fwd_lens_equals_attn_fwd_with_the_prefix_mask, their bf16 copies, and the qk-norm / rotary inputs of
    the fused epilogue (bit-equality does not need them to be consistent with q and k)"""
    def build():
        gen = torch.Generator().manual_seed(Np)
        q, k, v = ((torch.randn(Bq, H, Np, 64, generator=gen) * s).half().to(dev) for s in (1.5, 1.0, 1.0))
        _, rc, rs = rot_tables(Np, 16)
        return dict(q=q, k=k, v=v, qb=bf(q.float()), kb=bf(k.float()), vb=bf(v.float()), rc=rc.float().to(dev), rs=rs.float().to(dev),
                    rn=(0.05 + 0.1 * torch.rand(2, Bq, H, Np, generator=gen)).to(dev), gam=(1 + 0.2 * torch.randn(2, H, 64, generator=gen)).to(dev),
                    dout=bf(torch.randn(Bq, Np, I, generator=gen)).to(dev))
    return cached(("ops", Np), build)


def _forward(Np, klens):
    """vbx_attn_fwd_lens -> (out16, lse, key_lens, prefix mask, dout with the rows >= key_lens[b] zeroed)"""
    def build():
        from voicebox_pytorch_amd import _lib as L

        c = _operands(Np)
        kl = torch.tensor(klens, dtype=torch.int32, device=dev)
        mask = (torch.arange(Np, device=dev)[None] < kl[:, None]).contiguous()
        o16, lse = torch.empty(Bq, Np, I, dtype=torch.float16, device=dev), torch.empty(Bq, H, Np, device=dev)
        L.call("vbx_attn_fwd_lens", c["q"], c["k"], c["v"], mask, kl, o16, None, lse, Bq, H, Np, 10.0, _st())
        dout = (c["dout"] * mask[:, :, None]).contiguous()
        return o16, lse, kl, mask, dout
    return cached(("fwd", Np, klens), build)


def _bwd(Np, klens, name, mask_mode):
    """One unfused backward into NaN-filled buffers with a guard row -> (dq, dk, dv) incl. the guard.  mask_mode: "prefix" / None."""
    from voicebox_pytorch_amd import _lib as L

    c = _operands(Np)
    o16, lse, kl, mask, dout = _forward(Np, klens)
    m = mask if mask_mode == "prefix" else None
    dq, dk = nans((Bq * H * Np + 1, 64), torch.float32), nans((Bq * H * Np + 1, 64), torch.float32)
    dv = nans((Bq * Np + 1, I), torch.bfloat16)
    delta = torch.empty(Bq, H, Np, device=dev)
    head = (c["q"], c["k"], c["qb"], c["kb"], c["vb"], m)
    tail = (o16, 1, dout, lse, delta, dq, dk, dv, I, Bq, H, Np, 10.0, None, _st())
    if name == "vbx_attn_bwd":
        L.call(name, *head, *tail)
    else:
        L.call(name, *head, kl, *tail)
    torch.cuda.synchronize()
    return dq, dk, dv


def _bwd_fused(Np, klens, name, mask_mode, qknorm):
    """One fused backward -> (dqkv incl. guard row, gpart incl. guard record)"""
    from voicebox_pytorch_amd import _lib as L

    c = _operands(Np)
    o16, lse, kl, mask, dout = _forward(Np, klens)
    m = mask if mask_mode == "prefix" else None
    tiles = L.lib().vbx_attn_bwd_fused_tiles(Np)
    dqkv = nans((Bq * Np + 1, 3 * I), torch.bfloat16)
    gp = nans((2 * Bq * tiles + 1, H, 64), torch.float32)
    delta = torch.empty(Bq, H, Np, device=dev)
    head = (c["q"], c["k"], c["qb"], c["kb"], c["vb"], m)
    tail = (o16, 1, dout, lse, delta, c["rn"][0], c["rn"][1], c["gam"][0], c["gam"][1], c["rc"], c["rs"], 8.0 if qknorm else 0.0, dqkv,
            3 * I, gp, Bq, H, Np, 10.0, None, _st())
    if name == "vbx_attn_bwd_fused":
        L.call(name, *head, *tail)
    else:
        L.call(name, *head, kl, *tail)
    torch.cuda.synchronize()
    return dqkv, gp


# ------------------------------------------------------------------------------------------------ 1: the unfused entry point
@pytest.mark.parametrize("Np", [216, 272])
def test_attn_bwd_lens_equals_attn_bwd_with_the_prefix_mask(Np):
    """vbx_attn_bwd_lens (mask = the prefix mask, and mask = NULL) against vbx_attn_bwd with the prefix mask: dq, dk, dv rows
    < key_lens[b] have the same bits, rows >= key_lens[b] are == 0, the guard rows are still NaN; a rerun repeats bit for bit."""
    for klens in key_sets(Np):
        want = _bwd(Np, klens, "vbx_attn_bwd", "prefix")
        for mode in ("prefix", None):
            got = _bwd(Np, klens, "vbx_attn_bwd_lens", mode)
            for g, w, name in zip(got, want, ("dq", "dk", "dv")):
                assert g[-1].isnan().all() and w[-1].isnan().all(), (klens, mode, name)  # nothing past the end
                assert not g[:-1].isnan().any(), (klens, mode, name)                     # every row < Np is written
                heads = name != "dv"
                g4 = g[:-1].view(Bq, H, Np, 64) if heads else g[:-1].view(Bq, 1, Np, I)
                w4 = w[:-1].view(Bq, H, Np, 64) if heads else w[:-1].view(Bq, 1, Np, I)
                for b, kl in enumerate(klens):
                    assert same_bits(g4[b, :, :kl], w4[b, :, :kl]), (klens, mode, name, b)
                    assert (g4[b, :, kl:] == 0).all(), (klens, mode, name, b)
        again = _bwd(Np, klens, "vbx_attn_bwd_lens", "prefix")
        assert all(same_bits(a, g) for a, g in zip(again, got))
    print(f"PARITY attn_bwd_lens Np {Np}: dq / dk / dv bit-equal to the masked kernel on live rows, 0 beyond, over {key_sets(Np)}")


# ------------------------------------------------------------------------------------------------ 2: the fused entry point
@pytest.mark.parametrize("qknorm", [True, False])
@pytest.mark.parametrize("Np", [216, 272])
def test_attn_bwd_fused_lens_equals_attn_bwd_fused_with_the_prefix_mask(Np, qknorm):
    """vbx_attn_bwd_fused_lens against vbx_attn_bwd_fused with the mask: dqkv rows as above (q | k | v columns), gpart records bit-equal
    and zero in wholly dead tiles, gamma gradients (the records summed in order) bit-equal.  Without qk-norm no record is written."""
    from voicebox_pytorch_amd import _lib as L

    tiles = L.lib().vbx_attn_bwd_fused_tiles(Np)
    for klens in key_sets(Np):
        wd, wg = _bwd_fused(Np, klens, "vbx_attn_bwd_fused", "prefix", qknorm)
        for mode in ("prefix", None):
            gd, gg = _bwd_fused(Np, klens, "vbx_attn_bwd_fused_lens", mode, qknorm)
            assert gd[-1].isnan().all() and gg[-1].isnan().all() and not gd[:-1].isnan().any(), (klens, mode)
            g3, w3 = gd[:-1].view(Bq, Np, 3 * I), wd[:-1].view(Bq, Np, 3 * I)
            for b, kl in enumerate(klens):
                assert same_bits(g3[b, :kl], w3[b, :kl]), (klens, mode, b)
                assert (g3[b, kl:] == 0).all(), (klens, mode, b)
            assert same_bits(gg, wg), (klens, mode)  # without qk-norm: both untouched (NaN fill)
            if qknorm:
                rec = gg[:-1].view(2, Bq, tiles, H, 64)
                assert not rec.isnan().any()
                for b, kl in enumerate(klens):
                    dead0 = -(-kl // 128)  # the first 128-row tile wholly past the length
                    assert (rec[:, b, dead0:] == 0).all(), (klens, mode, b)
                assert same_bits(gg[:-1].view(2, Bq * tiles, H, 64).sum(1), wg[:-1].view(2, Bq * tiles, H, 64).sum(1))
    print(f"PARITY attn_bwd_fused_lens Np {Np} qk-norm {qknorm}: dqkv and gpart bit-equal to the masked kernel, over {key_sets(Np)}")


# ------------------------------------------------------------------------------------------------ 3: all rows full
@pytest.mark.parametrize("Np", [216, 272])
def test_full_lengths_without_a_mask_equal_the_plain_call(Np):
    """every key_lens[b] = Np, mask NULL: all outputs (guard rows included) are bit-equal to the plain unmasked call"""
    full = (Np,) * Bq
    for a, b in zip(_bwd(Np, full, "vbx_attn_bwd_lens", None), _bwd(Np, full, "vbx_attn_bwd", None)):
        assert same_bits(a, b)
    for qknorm in (True, False):
        for a, b in zip(_bwd_fused(Np, full, "vbx_attn_bwd_fused_lens", None, qknorm), _bwd_fused(Np, full, "vbx_attn_bwd_fused", None, qknorm)):
            assert same_bits(a, b)


def test_the_unfolded_bodies_fall_back_to_the_mask_bytes():
    """vbx_attn_bwd_select(3) has no length-aware kernel: vbx_attn_bwd_lens then runs the masked kernel on the prefix mask (the bits of
    vbx_attn_bwd under the same selection, guard rows included) and refuses a NULL mask instead of dropping the lengths."""
    from voicebox_pytorch_amd import _lib as L

    Np, klens = 216, (65, 128, 129)
    L.lib().vbx_attn_bwd_select(3)
    try:
        want, got = _bwd(Np, klens, "vbx_attn_bwd", "prefix"), _bwd(Np, klens, "vbx_attn_bwd_lens", "prefix")
        assert all(same_bits(g, w) for g, w in zip(got, want))
        with pytest.raises(L.VbxError, match="need the prefix mask bytes"):
            _bwd(Np, klens, "vbx_attn_bwd_lens", None)
    finally:
        L.lib().vbx_attn_bwd_select(0)


@pytest.mark.parametrize("Np", [216, 272])
def test_attn_fwd_lens_needs_no_mask_bytes(Np):
    """What the training forward launches: vbx_attn_fwd_lens with mask NULL writes the bits it writes with the prefix mask beside
    the lengths (output and lse, every row)."""
    from voicebox_pytorch_amd import _lib as L

    c = _operands(Np)
    for klens in key_sets(Np):
        o16, lse, kl, mask, _ = _forward(Np, klens)
        o2, l2 = torch.empty_like(o16), torch.empty_like(lse)
        L.call("vbx_attn_fwd_lens", c["q"], c["k"], c["v"], None, kl, o2, None, l2, Bq, H, Np, 10.0, _st())
        torch.cuda.synchronize()
        assert same_bits(o2, o16) and same_bits(l2, lse), klens


# ------------------------------------------------------------------------------------------------ 4: the model
SHAPES = [(3, 63), (2, 129), (5, 257), (4, 200)]


def _state():
    def build():
        cfg = restate.Cfg(dim=64, depth=2, heads=2, dim_head=64)
        state = restate.init_state_dict(cfg, seed=31)
        return cfg, {k: (v * 0.25 if k.endswith("q_norm.gamma") or k.endswith("k_norm.gamma") else v) for k, v in state.items()}
    return cached("state", build)


def _draws(B, N):
    """the setup of test_training_step_over_ragged_shapes_vs_oracle: row 0 full, the last row ONE frame when B > 2"""
    def build():
        gen = torch.Generator().manual_seed(1000 * B + N)
        x1, x0 = torch.randn(B, N, 64, generator=gen), torch.randn(B, N, 64, generator=gen)
        times, frac, rand = torch.rand(B, generator=gen), 0.7 + 0.3 * torch.rand(B, generator=gen), torch.rand(B, generator=gen)
        lengths = torch.randint(max(1, N // 3), N + 1, (B,), generator=gen)
        lengths[0] = N
        if B > 2:
            lengths[-1] = 1
        return x1, x0, times, frac, rand, lengths
    return cached(("draws", B, N), build)


def _model(**kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False, **kw)
    state = _state()[1]
    if kw.get("use_gateloop_layers"):
        state = dict(restate.init_state_dict(restate.Cfg(dim=64, depth=2, heads=2, dim_head=64, use_gateloop=True), seed=31))
        state = {k: (v * 0.25 if k.endswith("q_norm.gamma") or k.endswith("k_norm.gamma") else v) for k, v in state.items()}
    vb.load_state_dict(state, strict=False)
    vb = vb.to(dev)
    return vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, seed=None, **kw):
    from voicebox_pytorch_amd.masks import rng_override

    vb.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)  # the Philox key of a dropout forward is drawn from torch's CPU generator
    with rng_override(x0=x0, times=times, frac_lengths=frac, rand=rand):
        loss = wrapper(x1.to(dev), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in vb.named_parameters() if p.grad is not None}


def _assert_same(a, b, what):
    (la, ga), (lb, gb) = a, b
    assert same_bits(la, lb), (what, float(la), float(lb))
    assert ga.keys() == gb.keys()
    bad = [k for k in ga if not same_bits(ga[k], gb[k])]
    assert not bad, (what, [(k, float((ga[k] - gb[k]).abs().max())) for k in bad])


@pytest.mark.parametrize("B,N", SHAPES)
def test_lens_training_step_is_bit_equal_to_the_masked_step_and_meets_the_oracle(B, N):
    """loss and EVERY parameter gradient of wrapper(x1, lens=lengths) bit-equal to wrapper(x1, mask=prefix) with the same draws, and
    both within the bounds of test_training_step_over_ragged_shapes_vs_oracle of the fp64 restatement (loss 1e-3, gradients 0.04)."""
    x1, x0, times, frac, rand, lengths = _draws(B, N)
    mask = torch.arange(N)[None, :] < lengths[:, None]
    vb, wrapper = _model()
    by_mask = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, mask=mask.to(dev))
    by_lens = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, lens=lengths.tolist())
    _assert_same(by_lens, by_mask, (B, N))
    cfg, state = _state()
    p = {k: v.double().clone().requires_grad_(v.is_floating_point() and k != "null_cond") for k, v in state.items()}
    ref = restate.cfm_loss(p, cfg, x1.double(), x0.double(), times.double(), frac, rand, mask=mask)
    ref.backward()
    loss, grads = by_lens
    worst = max((rel(g, p[k].grad), k) for k, g in grads.items() if p[k].grad is not None and float(p[k].grad.norm()) > 0)
    print(f"PARITY train lens B {B} N {N} lengths {lengths.tolist()}: bit-equal to mask=; loss {float(loss):.6f} vs fp64 {float(ref.detach()):.6f}, "
          f"worst gradient rel {worst[0]:.2e} ({worst[1]})")
    assert abs(float(loss) - float(ref.detach())) < 1e-3, (float(loss), float(ref.detach()))
    for k, g in grads.items():
        if p[k].grad is not None and float(p[k].grad.norm()) > 0:
            assert rel(g, p[k].grad) < 0.04, (k, rel(g, p[k].grad))


@pytest.mark.parametrize("kw", [dict(attn_dropout=0.1), dict(use_gateloop_layers=True)], ids=["attn_dropout", "gateloop"])
def test_lens_training_step_on_the_fallback_and_gateloop_paths(kw):
    """The same bit-equality once with attn_dropout = 0.1 (no length-aware kernel: the masked kernels on the equivalent mask bytes, the
    same Philox seed in both arms) and once with use_gateloop_layers=True (the scan is causal: padding at the end reaches no live
    frame).  (The fp64 bounds of the plain model are not those of these two: dropout has no restated mask here, and the GateLoop
    oracle is held to looser bounds in test_model_gpu.py.)"""
    B, N = 4, 200
    x1, x0, times, frac, rand, lengths = _draws(B, N)
    mask = torch.arange(N)[None, :] < lengths[:, None]
    vb, wrapper = _model(**kw)
    by_mask = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, seed=5, mask=mask.to(dev))
    by_lens = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, seed=5, lens=lengths.tolist())
    _assert_same(by_lens, by_mask, kw)
    assert torch.isfinite(by_lens[0]) and all(torch.isfinite(g).all() for g in by_lens[1].values())
    print(f"PARITY train lens {kw}: loss {float(by_lens[0]):.6f} and every gradient bit-equal to mask=")


def test_train_step_with_lens_and_a_length_bucket_updates_like_the_masked_step():
    """TrainStep.step(lens=) with length_bucket=64 at N = 200 (run at 256 frames: the padding up to the bucket lies past every
    length): the loss and the updated parameters are bit-equal to the mask= step."""
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override

    B, N = 4, 200
    x1, x0, times, frac, rand, lengths = _draws(B, N)
    mask = torch.arange(N)[None, :] < lengths[:, None]
    out = []
    for kw in (dict(mask=mask.to(dev)), dict(lens=lengths)):
        vb, wrapper = _model()
        ts = TrainStep(wrapper, lr=1e-3, max_grad_norm=0.5, length_bucket=64)
        with rng_override(x0=x0, times=times, frac_lengths=frac, rand=rand):
            loss = ts.step(x1.to(dev), **kw)
        torch.cuda.synchronize()
        assert ts._last_eng.N == 256 and bool(ts._last_eng.io.key_lens) == ("lens" in kw)  # the lengths reached the runtime
        out.append((loss.detach().clone(), {k: v.detach().clone() for k, v in vb.state_dict().items()}))
    (lm, sm), (ll, sl) = out
    assert same_bits(lm, ll), (float(lm), float(ll))
    assert all(same_bits(sm[k], sl[k]) for k in sm), [k for k in sm if not same_bits(sm[k], sl[k])]
    state = _state()[1]
    assert any(not torch.equal(sl[k].cpu(), state[k]) for k in state if k in sl and state[k].is_floating_point())  # the step moved them
    print(f"PARITY TrainStep.step(lens=) length_bucket 64, N 200 -> 256: loss {float(ll):.6f}, updated parameters bit-equal to mask=")


# ------------------------------------------------------------------------------------------------ 5: padding cannot leak
def test_padding_cannot_leak_into_the_lens_step():
    """The lens= step twice, the second time with 1e3 * randn planted past the lengths in x1 and in the x0 draw: loss and gradients
    have the same bits -- any kernel that reads a padding frame into a live sum fails this."""
    B, N = 4, 200
    x1, x0, times, frac, rand, lengths = _draws(B, N)
    lens = lengths.tolist()
    gen = torch.Generator().manual_seed(77)
    vb, wrapper = _model()
    a = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, lens=lens)
    b = _loss_and_grads(vb, wrapper, plant(x1, lens, gen), plant(x0, lens, gen), times, frac, rand, lens=lens)
    _assert_same(b, a, "planted")


# ------------------------------------------------------------------------------------------------ 6: unchecked device lengths
def test_a_device_lens_tensor_is_clamped_on_the_device():
    """A device lens tensor holding 0 and N + 5 runs as if it held 1 and N -- equal to the clamped list -- and neither faults nor raises."""
    B, N = 4, 200
    x1, x0, times, frac, rand, lengths = _draws(B, N)
    raw = lengths.clone()
    raw[1], raw[2] = 0, N + 5
    vb, wrapper = _model()
    a = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, lens=raw.clamp(1, N).tolist())
    b = _loss_and_grads(vb, wrapper, x1, x0, times, frac, rand, lens=raw.to(dev))
    _assert_same(b, a, "clamped")
    assert torch.isfinite(b[0])
