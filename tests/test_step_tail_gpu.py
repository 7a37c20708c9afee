"""GPU: the once-per-step launches of the train step that were folded into fewer launches, each against the entry points it replaces.

Every folded form runs the device bodies of the launches it stands for, in the same order per element, so every comparison here is
torch.equal -- no tolerance:
  vbx_embed_bwd_tail1 / _tail2 / _wsin  vs  vbx_stack_input_bwd's dreg, vbx_conv_wgrad_finalize, vbx_time_embed_bwd, vbx_splitk_reduce, vbx_colsum_f32
  vbx_span_masks / vbx_cfm_inputs_masks vs  masks.mask_from_frac_lengths, the loss-mask expression and vbx_cfm_inputs
  two TrainStep.step calls              vs  the same tree with both folded paths bypassed through the old entry points
Sizes sit off the block sizes (D = 80, 3 chunks, B = 3, Th = 96, 37 frames behind 16 register rows).
(The issue's other merges -- zero rows written by the final norm's backward, its gamma gradient in layer 0's batched reduce, the clip
norm in two launches, the loss in one -- were measured or priced and left out; their comparisons went with them.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape):
    return torch.randn(*shape, generator=g).to(dev)


# ------------------------------------------------------------------------------------------------ embed backward finishers
def test_embed_bwd_tails(L):
    """the two grouped launches + vbx_time_embed_bwd_wsin against the launches of vbx_model_backward_embed that they stand for"""
    B, N, R, D, Th, ks, chunks, splits, Ke = 3, 37, 16, 80, 96, 31, 3, 3, 168
    Np, M0 = N + R, B * N
    g = gen(31)
    lib = L.lib()
    dxs, wpart = rnd(g, B, Np, D), rnd(g, chunks, D, 64)
    times, wsin, w1 = torch.rand(B, generator=g).to(dev), rnd(g, D // 2), rnd(g, Th, D)
    four, pre, dtemb = rnd(g, B, D), rnd(g, B, Th), rnd(g, B, Th)
    slabs, de = rnd(g, splits, D, Ke), rnd(g, M0, D)
    nts = lib.vbx_time_embed_bwd_scratch_floats(B, D)
    ncs = lib.vbx_colsum_scratch_floats(M0, D)

    def nan(*shape):
        return torch.full(shape, float("nan"), device=dev)

    def outputs():
        return dict(dreg=nan(R, D), dw=nan(D, ks), db=nan(D), dw1=nan(Th, D), db1=nan(Th), dwsin=nan(D // 2), ts=nan(nts), dembw=nan(D, Ke),
                    dembb=nan(D), cs=nan(ncs))

    r = outputs()
    L.call("vbx_stack_input_bwd", dxs, nan(B, N, D), r["dreg"], B, N, R, D, st())
    L.call("vbx_conv_wgrad_finalize", wpart, chunks, D, ks, r["dw"], r["db"], st())
    L.call("vbx_time_embed_bwd", times, wsin, w1, four, pre, dtemb, r["dwsin"], r["dw1"], r["db1"], r["ts"], B, D, Th, st())
    L.call("vbx_splitk_reduce", slabs, splits, D, Ke, r["dembw"], D, Ke, Ke, 0, 0, 0, st())
    L.call("vbx_colsum_f32", de, M0, D, D, r["dembb"], r["cs"], st())
    o = outputs()
    L.call("vbx_embed_bwd_tail1", dxs, o["dreg"], B, Np, R, D, wpart, chunks, ks, o["dw"], o["db"], four, pre, dtemb, w1, o["dw1"], o["db1"],
           o["ts"], Th, st())
    L.call("vbx_colsum_f32_partials", de, M0, D, D, o["cs"], st())
    L.call("vbx_embed_bwd_tail2", slabs, splits, D, Ke, o["dembw"], o["cs"], D, o["dembb"], o["ts"], B, D, st())
    L.call("vbx_time_embed_bwd_wsin", times, four, o["ts"], o["dwsin"], B, D, st())
    torch.cuda.synchronize()
    for k in r:
        assert torch.isfinite(r[k]).all(), k
        assert torch.equal(o[k], r[k]), k
    # no register tokens: the first group runs without that job
    o2 = outputs()
    L.call("vbx_embed_bwd_tail1", dxs, None, B, N, 0, D, wpart, chunks, ks, o2["dw"], o2["db"], four, pre, dtemb, w1, o2["dw1"], o2["db1"], o2["ts"],
           Th, st())
    torch.cuda.synchronize()
    for k in ("dw", "db", "dw1", "db1"):
        assert torch.equal(o2[k], r[k]), k
    assert torch.equal(o2["ts"][B * D:], r["ts"][B * D:])


# ------------------------------------------------------------------------------------------------ masks
def _python_masks(N, frac, rand, pad, lens):
    from voicebox_pytorch_amd.masks import mask_from_frac_lengths, rng_override

    with rng_override(rand=rand):
        cond = mask_from_frac_lengths(N, frac)
    loss = cond
    if pad is not None:
        loss = loss & pad
    if lens is not None:
        loss = loss & (torch.arange(N, device=dev)[None, :] < lens[:, None])
    return cond, loss


@pytest.mark.parametrize("with_lens", [False, True], ids=["nolens", "lens"])
@pytest.mark.parametrize("with_pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("N", [1, 37, 256])
def test_span_masks(L, N, with_pad, with_lens):
    R = 16
    g = gen(41 + N)
    # rows: frac 0, 0.7 and 1.0 with rand 0, just under 1 and random, then random rows
    frac = torch.cat([torch.tensor([0.0, 0.7, 1.0]).repeat_interleave(3), 0.7 + 0.3 * torch.rand(23, generator=g), torch.rand(8, generator=g)])
    B = frac.numel()
    rand = torch.rand(B, generator=g)
    rand[0:9:3], rand[1:9:3] = 0.0, float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    frac, rand = frac.to(dev), rand.to(dev)
    pad = (torch.rand(B, N, generator=g) < 0.8).to(dev) if with_pad else None
    lens = None
    if with_lens:
        lens = torch.randint(0, N + 1, (B,), generator=g).to(dev)
        lens[1], lens[2] = 0, N  # a row with no frame at all, a full one
    key_lens = (lens + R).to(torch.int32) if with_lens else None
    cond_ref, loss_ref = _python_masks(N, frac, rand, pad, lens)
    cond = torch.full((B, N), True, device=dev)
    loss = torch.full((B, N), True, device=dev)
    L.call("vbx_span_masks", frac, rand, pad, key_lens, R, B, N, cond, loss, st())
    torch.cuda.synchronize()
    assert torch.equal(cond, cond_ref) and torch.equal(loss, loss_ref)
    assert bool((cond.view(torch.uint8) <= 1).all()) and bool((loss.view(torch.uint8) <= 1).all())  # proper bool storage
    if N > 1:
        assert bool(cond_ref.any()) and not bool(cond_ref.all())
    # the same in the grid of vbx_cfm_inputs, with that kernel's outputs
    Dl = 12
    x1, x0, times = rnd(g, B, N, Dl), rnd(g, B, N, Dl), torch.rand(B, generator=g).to(dev)
    w_ref, f_ref = torch.full_like(x1, float("nan")), torch.full_like(x1, float("nan"))
    L.call("vbx_cfm_inputs", x1, x0, times, 1e-5, w_ref, f_ref, B, N * Dl, st())
    w, f = torch.full_like(x1, float("nan")), torch.full_like(x1, float("nan"))
    cond2, loss2 = torch.full((B, N), True, device=dev), torch.full((B, N), True, device=dev)
    L.call("vbx_cfm_inputs_masks", x1, x0, times, 1e-5, w, f, B, N * Dl, frac, rand, pad, key_lens, R, N, cond2, loss2, st())
    torch.cuda.synchronize()
    assert torch.isfinite(w_ref).all() and torch.equal(w, w_ref) and torch.equal(f, f_ref)
    assert torch.equal(cond2, cond_ref) and torch.equal(loss2, loss_ref)


def test_span_masks_without_a_loss_mask(L):
    frac, rand = torch.tensor([0.8], device=dev), torch.tensor([0.5], device=dev)
    cond = torch.zeros(1, 40, dtype=torch.bool, device=dev)
    L.call("vbx_span_masks", frac, rand, None, None, 0, 1, 40, cond, None, st())
    torch.cuda.synchronize()
    assert torch.equal(cond, _python_masks(40, frac, rand, None, None)[0])


# ------------------------------------------------------------------------------------------------ the whole step
def _old_inputs_and_masks(self, x1, x0, times, frac, mask, key_lens):
    """TrainStep._cfm_inputs_and_masks as it was: vbx_cfm_inputs, then the masks with torch"""
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.masks import mask_from_frac_lengths

    B, N, _ = x1.shape
    wt, flow = torch.empty_like(x1), torch.empty_like(x1)
    _lib.call("vbx_cfm_inputs", x1, x0.contiguous(), times.contiguous(), float(self.wrapper.sigma), wt, flow, B, x1[0].numel(), st())
    cond_mask = mask_from_frac_lengths(N, frac)
    return wt, flow, cond_mask, (cond_mask if mask is None else (cond_mask & mask))


def _two_steps(heads, with_mask, folded, monkeypatch):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override
    from oracle import restate

    dim, depth, B, N = 64, 2, 2, 40
    cfg = restate.Cfg(dim=dim, depth=depth, heads=heads, dim_head=64)
    state = restate.init_state_dict(cfg, seed=5)
    g = gen(77)
    for k in sorted(state):  # the adaLN projections start at zero: move them, so that every gradient carries signal
        if ".to_gamma." in k or ".to_beta." in k:
            state[k] = state[k] + 0.05 * torch.randn(state[k].shape, generator=g)
    vb = vbx.VoiceBox(dim=dim, num_cond_tokens=5, depth=depth, dim_head=64, heads=heads, condition_on_text=False)
    vb.load_state_dict(state, strict=False)
    ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev)), lr=1e-3, max_grad_norm=0.5)
    calls = []
    if not folded:  # the test's own switch: both folded paths go back through the entry points they replaced
        monkeypatch.setattr(TrainStep, "_cfm_inputs_and_masks", _old_inputs_and_masks)
    else:
        inner = TrainStep._cfm_inputs_and_masks
        monkeypatch.setattr(TrainStep, "_cfm_inputs_and_masks", lambda self, *a, **k: (calls.append("masks"), inner(self, *a, **k))[1])
    _lib.call("vbx_embed_tail_grouped", 1 if folded else 0)
    out = []
    try:
        for i in range(2):
            x1 = torch.randn(B, N, dim, generator=g).to(dev)
            draws = dict(x0=torch.randn(B, N, dim, generator=g), times=torch.rand(B, generator=g),
                         frac_lengths=0.7 + 0.3 * torch.rand(B, generator=g), rand=torch.rand(B, generator=g))
            mask = None
            if with_mask:
                mask = (torch.arange(N)[None, :] < torch.tensor([N, N - 7])[:, None]).to(dev)
            with rng_override(**draws):
                loss = ts.step(x1, mask=mask)
            torch.cuda.synchronize()
            out.append((loss.clone(), ts.fp.flat.detach().clone(), ts.coef.clone(), ts.sumsq.clone()))
    finally:
        _lib.call("vbx_embed_tail_grouped", 1)
    if folded:
        assert calls == ["masks"] * 2  # the path that was meant is the path that ran
    return out


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("heads", [2, 4])  # (VoiceBox refuses an odd head count, so one head cannot be built: two and four)
def test_two_steps_equal_the_unfolded_paths(L, heads, with_mask, monkeypatch):
    got = _two_steps(heads, with_mask, True, monkeypatch)
    monkeypatch.undo()
    ref = _two_steps(heads, with_mask, False, monkeypatch)
    for i, (a, b) in enumerate(zip(got, ref)):
        for name, x, y in zip(("loss", "params", "coef", "sumsq"), a, b):
            assert torch.isfinite(y).all(), (i, name)
            assert torch.equal(x, y), (i, name, float((x - y).abs().max()))
    assert not torch.equal(ref[0][1], ref[1][1])  # the second step moved the parameters again
