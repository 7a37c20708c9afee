"""VoiceBox(audio_enc_dec=codec) with latent_dim != dim on the device: the model path against the unmodified reference (fixtures
small_codec / small_codec_text of tests/golden/make_golden_codec.py) with the bounds of the dim_in test (test_model_gpu.py: loss
1e-3, every gradient rel < 0.03, prediction 0.01, sample 0.02), the fused proj_in kernel and its weight gradient against fp64 with
DERIVED bounds, the optimizer / trainer round trips, and latent_dim == dim against the same model without a codec."""
import ctypes as C
import os

import pytest
import torch

import codec_ref
import ode_ref
from oracle import restate
from toy_codec import ToyCodec

pytestmark = pytest.mark.gpu
dev = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def _grads(name):
    return torch.load(os.path.join(GOLDEN, name + "_grads.pt"), map_location="cpu", weights_only=False)


def _build(g, text=False):
    import voicebox_pytorch_amd as vbx

    kw = dict(num_cond_tokens=50, dim_cond_emb=48, condition_on_text=True) if text else dict(num_cond_tokens=500, condition_on_text=False)
    vb = vbx.VoiceBox(dim=64, audio_enc_dec=ToyCodec(g["latent_dim"]), depth=2, dim_head=64, heads=2, time_hidden_dim=g["time_hidden_dim"],
                      ff_mult=g["ff_mult"], **kw)
    missing = vb.load_state_dict(g["state"], strict=False)
    assert not missing.unexpected_keys and all("inv_freq" in k for k in missing.missing_keys), missing
    return vb.to(dev)


def test_codec_model_vs_reference(golden):
    """latent 100 into dim 64, trained from a wave: loss, every gradient (proj_in.weight / proj_in.bias among them), the mixed call
    wrapper(latents, cond=wave), an eval prediction at two times, a 5-point midpoint sample (eager and under hipGraph) to latents and
    decoded to a wave -- against the unmodified reference."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g, grads = golden("small_codec"), _grads("small_codec")
    vb = _build(g)
    assert vb.proj_in.weight.shape == (64, 100) and vb.to_embed.weight.shape == (64, 128) and vb.to_pred.weight.shape == (100, 64)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    with rng_override(x0=g["x0"], times=g["times"], frac_lengths=g["frac"], rand=g["rand"]):
        loss = wrapper(g["wave"].to(dev))
    loss.backward()
    print("small_codec loss", float(loss.detach()), "reference", float(g["loss"]))
    assert abs(float(loss) - float(g["loss"])) < 1e-3, (float(loss), float(g["loss"]))
    named = dict(vb.named_parameters())
    assert "proj_in.weight" in grads and "proj_in.bias" in grads
    worst = max((rel(named[k].grad, ref), k) for k, ref in grads.items())
    print("small_codec worst gradient", worst, "proj_in.weight", rel(named["proj_in.weight"].grad, grads["proj_in.weight"]),
          "proj_in.bias", rel(named["proj_in.bias"].grad, grads["proj_in.bias"]))
    for k, ref in grads.items():
        assert rel(named[k].grad, ref) < 0.03, (k, rel(named[k].grad, ref))
    with rng_override(x0=g["x0"], times=g["times"], frac_lengths=g["frac"], rand=g["rand"]):
        loss_m = wrapper(g["lat1"].to(dev), cond=g["wave_cond"].to(dev))
    assert abs(float(loss_m) - float(g["loss_mixed"])) < 1e-3, (float(loss_m), float(g["loss_mixed"]))
    del loss_m
    vb.eval()
    cond = vb.audio_enc_dec.encode(g["wave_cond"].to(dev))
    with torch.no_grad():
        pred = vb(g["lat1"].to(dev), times=g["eval_times"].to(dev), cond_token_ids=None, cond=cond, cond_drop_prob=0.0)
    print("small_codec pred rel", rel(pred, g["pred"]))
    assert pred.shape == (2, 40, 100) and rel(pred, g["pred"]) < 0.01, rel(pred, g["pred"])
    for graph in (False, True):
        with rng_override(y0=g["y0"]):
            s5 = wrapper.sample(cond=g["wave_cond"].to(dev), steps=5, use_graph=graph, decode_to_audio=False)
        print("small_codec sample rel", graph, rel(s5, g["sample5"]))
        assert s5.shape == (2, 40, 100) and rel(s5, g["sample5"]) < 0.02, (graph, rel(s5, g["sample5"]))
        with rng_override(y0=g["y0"]):
            wave = wrapper.sample(cond=g["wave_cond"].to(dev), steps=5, use_graph=graph)
        assert wave.shape == (2, 640) and rel(wave, g["sample5_wave"]) < 0.02, (graph, rel(wave, g["sample5_wave"]))
    with rng_override(y0=g["y0"]):
        codes = wrapper.sample(cond=g["wave_cond"].to(dev), steps=5, decode_to_codes=True)
    assert codes.shape == (2, 40) and codes.dtype == torch.int64
    with pytest.raises(NotImplementedError):
        wrapper(g["wave"].to(dev), input_sampling_rate=16000)


@pytest.mark.parametrize("method", ["euler", "rk4", "dopri5"])
@pytest.mark.parametrize("graph", [False, True])
def test_codec_model_other_ode_methods(golden, method, graph):
    """euler / rk4 / dopri5 at state width latent_dim against the CPU restatement (tests/ode_ref.py over tests/codec_ref.py, itself
    equal to the reference's prediction on the fixture: test_codec_cpu.py), same 0.02 as the midpoint sample."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_codec")
    vb = _build(g).eval()
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=method)
    cfg = restate.Cfg(dim=64, depth=2, heads=2, dim_head=64, ff_mult=g["ff_mult"])
    cond = ToyCodec(100).encode(g["wave_cond"])
    ones = torch.ones(2, 40, dtype=torch.bool)
    fn = lambda t, y: codec_ref.codec_forward(g["state"], cfg, y, t, cond, ones)
    with torch.no_grad():
        want = ode_ref.odeint(fn, g["y0"], torch.linspace(0, 1, 5), method=method)
    with rng_override(y0=g["y0"]):
        got = wrapper.sample(cond=g["wave_cond"].to(dev), steps=5, use_graph=graph, decode_to_audio=False)
    print("small_codec", method, graph, rel(got, want), wrapper.last_sample_stats)
    assert got.shape == (2, 40, 100) and rel(got, want) < 0.02, (method, graph, rel(got, want))


def test_codec_text_model_vs_reference(golden):
    """latent 128, text-conditioned, classifier-free drop replayed (one of three samples dropped: the null_cond branch of the fused
    kernel and of its gradient), guided sampling with cond=None (zeros of latent_dim) and from a wave."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g, grads = golden("small_codec_text"), _grads("small_codec_text")
    vb = _build(g, text=True)
    assert vb.proj_in.weight.shape == (64, 128) and vb.to_embed.weight.shape == (64, 176) and vb.null_cond.shape == (64,)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, cond_drop_prob=0.5)
    with rng_override(x0=g["x0"], times=g["times"], frac_lengths=g["frac"], rand=g["rand"], cond_drop=g["drop"]):
        loss = wrapper(g["wave"].to(dev), semantic_token_ids=g["ids"].to(dev))
    loss.backward()
    print("small_codec_text loss", float(loss.detach()), "reference", float(g["loss"]))
    assert abs(float(loss) - float(g["loss"])) < 1e-3, (float(loss), float(g["loss"]))
    named = dict(vb.named_parameters())
    print("small_codec_text worst gradient", max((rel(named[k].grad, ref), k) for k, ref in grads.items()))
    for k, ref in grads.items():
        assert rel(named[k].grad, ref) < 0.03, (k, rel(named[k].grad, ref))
    for graph in (False, True):
        with rng_override(y0=g["y0"]):
            s3 = wrapper.sample(cond=None, semantic_token_ids=g["ids"].to(dev), steps=3, cond_scale=1.3, use_graph=graph, decode_to_audio=False)
        print("small_codec_text sample(cond=None) rel", graph, rel(s3, g["sample3_nocond"]))
        assert s3.shape == (3, 40, 128) and rel(s3, g["sample3_nocond"]) < 0.02, (graph, rel(s3, g["sample3_nocond"]))
        with rng_override(y0=g["y0"]):
            w3 = wrapper.sample(cond=g["wave"].to(dev), semantic_token_ids=g["ids"].to(dev), steps=3, cond_scale=1.3, use_graph=graph)
        assert w3.shape == (3, 640) and rel(w3, g["sample3_wave"]) < 0.02, (graph, rel(w3, g["sample3_wave"]))


# ------------------------------------------------------------------------------------ the fused kernel alone
def _st():
    return torch.cuda.current_stream().cuda_stream


def _case(L, B, N, D, seed, mode):
    gen = torch.Generator().manual_seed(seed)
    x, cond = torch.randn(B, N, L, generator=gen), torch.randn(B, N, L, generator=gen)
    w, b = torch.randn(D, L, generator=gen) * L ** -0.5, torch.randn(D, generator=gen) * 0.1
    null = torch.randn(D, generator=gen)
    cm = torch.rand(B, N, generator=gen) < 0.6
    drop = None
    if mode == "all_masked":
        cm[0] = True
    elif mode == "none_masked":
        cm[0] = False
    elif mode == "dropped":
        drop = torch.zeros(B, dtype=torch.bool)
        drop[B - 1] = True
    return x, cond, w, b, null, cm, drop


def _run_kernel(x, cond, w, b, null, cm, drop, training=True):
    from voicebox_pytorch_amd import _lib as Lb

    B, N, L = x.shape
    D = w.shape[0]
    Kp = Lb.lib().vbx_proj_in_kp(L)
    assert Kp % 32 == 0 and Kp > L
    wh = torch.zeros(D, Kp, dtype=torch.float16)
    wh[:, :L] = w.to(torch.float16)
    out16 = torch.full((B * N, 2 * D), float("nan"), dtype=torch.float16, device=dev)
    outb = torch.full((B * N, 2 * D), float("nan"), dtype=torch.bfloat16, device=dev) if training else None
    xcb = torch.full((2 * B * N, Kp), float("nan"), dtype=torch.bfloat16, device=dev) if training else None
    keep = (x.to(dev).contiguous(), cond.to(dev).contiguous(), wh.to(dev), b.to(dev), cm.to(dev).view(torch.uint8),
            drop.to(dev).view(torch.uint8) if drop is not None else None, null.to(dev))
    Lb.call("vbx_proj_in_embed", keep[0], keep[1], keep[2], keep[3], keep[4], keep[5], keep[6], out16, outb, xcb, B, N, L, D, 0, _st())
    torch.cuda.synchronize()
    return out16, outb, xcb, Kp


CASES = [(L, B, N, mode) for L in (8, 100, 128, 1024) for (B, N) in ((1, 31), (2, 16), (1, 33), (3, 43), (2, 64), (1, 129))
         for mode in ("plain",)] + [(100, 3, 43, m) for m in ("all_masked", "none_masked", "dropped")] + \
        [(1024, 2, 65, "dropped"), (8, 2, 65, "all_masked")]


@pytest.mark.parametrize("L,B,N,mode", CASES)
def test_proj_in_embed_kernel_vs_fp64(L, B, N, mode):
    """Bound per element, derived (not measured): against fp64 on the UNROUNDED inputs, two fp16 operand roundings (2^-11 each, so
    2^-10 + 2^-22 on a product), K + 2 fp32 accumulation / bias roundings of 2^-24 on the running magnitude, then one output rounding
    (fp16: 2^-11 relative, 2^-24 absolute in the subnormal range; bf16: 2^-8).  Masked rows are exactly zero, dropped samples exactly
    null_cond rounded to the output format."""
    D = 128
    x, cond, w, b, null, cm, drop = _case(L, B, N, D, 1000 + L + 7 * B * N, mode)
    out16, outb, xcb, Kp = _run_kernel(x, cond, w, b, null, cm, drop)
    xp, cp = codec_ref.embed_operand(x, cond, w, b, cm, drop, null)
    sx = x.double().abs() @ w.double().abs().t() + b.double().abs()
    sc = cond.double().abs() @ w.double().abs().t() + b.double().abs()
    acc_bound = lambda s: (2.0 ** -10 + 2.0 ** -22 + (L + 2) * 2.0 ** -24) * s
    worst = 0.0
    for got, orel, oabs in ((out16, 2.0 ** -11, 2.0 ** -24), (outb, 2.0 ** -8, 0.0)):
        got = got.double().cpu().view(B, N, 2 * D)
        gx, gc = got[..., :D], got[..., D:]
        bx = acc_bound(sx)
        bx = bx + (xp.abs() + bx) * orel + oabs
        assert torch.isfinite(got).all()
        assert bool(((gx - xp).abs() <= bx).all()), float(((gx - xp).abs() / bx).max())
        worst = max(worst, float(((gx - xp).abs() / bx).max()))
        live = ~cm if drop is None else (~cm & ~drop[:, None])
        bc = acc_bound(sc)
        bc = bc + (cp.abs() + bc) * orel + oabs
        assert bool(((gc - cp).abs() <= bc)[live].all()), float(((gc - cp).abs() / bc)[live].max())
        masked = cm if drop is None else (cm & ~drop[:, None])
        assert bool((gc[masked] == 0).all())
        if drop is not None:
            want = null.to(torch.float16 if orel == 2.0 ** -11 else torch.bfloat16).double()
            assert bool((gc[drop] == want).all())
    # the weight-gradient operand: x rows, cond rows zeroed where no gradient passes, column L = 1 on the rows that count
    xc = xcb.float().cpu().view(2, B, N, Kp)
    live = ~cm if drop is None else (~cm & ~drop[:, None])
    assert torch.equal(xc[0, ..., :L], x.to(torch.bfloat16).float()) and bool((xc[0, ..., L] == 1).all()) and bool((xc[0, ..., L + 1:] == 0).all())
    assert torch.equal(xc[1, ..., :L], cond.to(torch.bfloat16).float() * live[..., None]) and torch.equal(xc[1, ..., L], live.float())
    assert bool((xc[1, ..., L + 1:] == 0).all())
    print(f"proj_in_embed L={L} B={B} N={N} {mode}: worst |err| / bound = {worst:.3f}")
    # inference: no bf16 copy, no gradient operand, same fp16 rows
    o2, _, _, _ = _run_kernel(x, cond, w, b, null, cm, drop, training=False)
    assert torch.equal(o2.view(torch.int16), out16.view(torch.int16))


@pytest.mark.parametrize("L,B,N,mode", [c for c in CASES if c[2] != 31 or c[0] == 100])
def test_proj_in_weight_gradient_vs_fp64(L, B, N, mode):
    """d(proj_in.weight) / d(proj_in.bias) = dY^T . xc through the split-K product and vbx_proj_in_wgrad_reduce, dY = [dx' ; dcond']
    exactly representable in bf16.  Derived bound: the one rounded operand (x to bf16: 2^-8 as the project counts a bf16 operand) plus
    K = 2 B N fp32 accumulations of 2^-24, times sum |dy . x|; the bias column multiplies by exact ones (accumulation term only)."""
    from voicebox_pytorch_amd import _lib as Lb

    D = 128
    x, cond, w, b, null, cm, drop = _case(L, B, N, D, 2000 + L + 7 * B * N, mode)
    _, _, xcb, Kp = _run_kernel(x, cond, w, b, null, cm, drop)
    M = B * N
    Mp = (2 * M + 7) // 8 * 8
    gen = torch.Generator().manual_seed(5)
    dy = torch.zeros(Mp, D)
    dy[:2 * M] = torch.randn(2 * M, D, generator=gen)
    dy = dy.to(torch.bfloat16)
    xcp = torch.zeros(Mp, Kp, dtype=torch.bfloat16, device=dev)
    xcp[:2 * M] = xcb
    dyd = dy.to(dev)
    splits = 2 if 2 * M >= 64 else 1
    slabs = torch.empty(splits, D, Kp, dtype=torch.float32, device=dev)
    gd = Lb.GemmDesc()
    gd.mode, gd.epilogue, gd.M, gd.N, gd.K, gd.lda, gd.ldb, gd.splits = Lb.VBX_GEMM_TN, Lb.VBX_EPI_SPLITK, D, Kp, Mp, D, Kp, splits
    gd.A, gd.B, gd.C = dyd.data_ptr(), xcp.data_ptr(), slabs.data_ptr()
    Lb.call("vbx_gemm", C.byref(gd), _st())
    dw, db = torch.empty(D, L, device=dev), torch.empty(D, device=dev)
    Lb.call("vbx_proj_in_wgrad_reduce", slabs, splits, D, L, dw, db, _st())
    torch.cuda.synchronize()
    dyf = dy[:2 * M].double().view(2, B, N, D)
    rw, rb = codec_ref.proj_in_grads(x, cond, dyf[0], dyf[1], cm, drop)
    keep = ~cm if drop is None else (~cm & ~drop[:, None])
    s = dyf[0].abs().reshape(M, D).t() @ x.double().abs().reshape(M, L) + (dyf[1].abs() * keep[..., None]).reshape(M, D).t() @ cond.double().abs().reshape(M, L)
    bw = (2.0 ** -8 + 2 * M * 2.0 ** -24) * s + 1e-30
    sb = dyf[0].abs().sum(dim=(0, 1)) + (dyf[1].abs() * keep[..., None]).sum(dim=(0, 1))
    bb = 2 * M * 2.0 ** -24 * sb + 1e-30
    ew, eb = (dw.double().cpu() - rw).abs(), (db.double().cpu() - rb).abs()
    print(f"proj_in wgrad L={L} B={B} N={N} {mode}: worst |err| / bound weight {float((ew / bw).max()):.3f} bias {float((eb / bb).max()):.3f}")
    assert bool((ew <= bw).all()), float((ew / bw).max())
    assert bool((eb <= bb).all()), float((eb / bb).max())


# ------------------------------------------------------------------------------------ optimizer / trainer / identity
def test_train_step_keeps_operand_copies_in_step(golden):
    """one TrainStep from a WAVE batch, then the state loaded into a fresh model: torch.equal predictions -- the fused Adam refreshed
    the padded operand copies of proj_in ([64, 128] from [64, 100]) and to_pred ([104, 64] from [100, 64]) in the same pass."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_codec")
    vb = _build(g)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    before = {k: v.detach().clone() for k, v in vb.state_dict().items()}
    ts = TrainStep(wrapper, lr=1e-3, max_grad_norm=0.5)
    with rng_override(x0=g["x0"], times=g["times"], frac_lengths=g["frac"], rand=g["rand"]):
        loss = ts.step(g["wave"].to(dev))
    assert abs(float(loss) - float(g["loss"])) < 1e-3
    sd = {k: v.detach().cpu().clone() for k, v in vb.state_dict().items()}
    for k in ("proj_in.weight", "proj_in.bias", "to_pred.weight", "to_embed.weight"):
        assert not torch.equal(sd[k], before[k].cpu()), k + " did not move"
    vb2 = _build(dict(g, state=sd)).eval()
    vb.eval()
    cond = vb.audio_enc_dec.encode(g["wave_cond"].to(dev))
    with torch.no_grad():
        p1 = vb(g["lat1"].to(dev), times=g["eval_times"].to(dev), cond_token_ids=None, cond=cond, cond_drop_prob=0.0)
        p2 = vb2(g["lat1"].to(dev), times=g["eval_times"].to(dev), cond_token_ids=None, cond=cond, cond_drop_prob=0.0)
    assert torch.equal(p1, p2)


def test_trainer_save_load_round_trip(golden, tmp_path):
    """VoiceBoxTrainer on a dataset of waves: two steps, save, load into a fresh trainer: same parameters (proj_in among them), same
    optimizer state, and the next step gives the same loss."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_codec")

    class Waves(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return torch.randn(640, generator=torch.Generator().manual_seed(i))

    def make(folder):
        wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=_build(g))
        return vbx.VoiceBoxTrainer(wrapper, batch_size=2, dataset=Waves(), num_train_steps=10, num_warmup_steps=2, lr=1e-3,
                                   valid_frac=0.25, results_folder=str(tmp_path / folder), log_every=100, save_results_every=100,
                                   save_model_every=100, force_clear_prev_results=True)

    torch.manual_seed(0)
    tr = make("a")
    tr.train_step()
    tr.train_step()
    path = str(tmp_path / "voicebox.2.pt")
    tr.save(path)
    tr2 = make("b")
    tr2.load(path)
    sd1, sd2 = tr.cfm_wrapper.state_dict(), tr2.cfm_wrapper.state_dict()
    assert "voicebox.proj_in.weight" in sd1
    for k in sd1:
        assert torch.equal(sd1[k].cpu(), sd2[k].cpu()), k
    wave = torch.randn(2, 640, generator=torch.Generator().manual_seed(99))
    lat = ToyCodec(100).encode(wave)
    draws = dict(x0=torch.randn(lat.shape, generator=torch.Generator().manual_seed(98)), times=torch.tensor([0.3, 0.6]),
                 frac_lengths=torch.tensor([0.8, 0.9]), rand=torch.tensor([0.2, 0.7]))
    losses = []
    for t in (tr, tr2):
        with rng_override(**draws):
            losses.append(float(t.train_step_fn.step(wave.to(dev), lr=1e-3)))
    assert losses[0] == losses[1], losses


def test_latent_dim_equal_to_dim_is_the_codec_free_path(golden):
    """latent_dim == dim: proj_in is nn.Identity and the engine takes exactly the code of a model without a codec -- bit-identical
    loss, gradients, prediction and sample."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    kw = dict(dim=64, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False, time_hidden_dim=64, ff_mult=2)
    torch.manual_seed(3)
    plain = vbx.VoiceBox(**kw)
    coded = vbx.VoiceBox(audio_enc_dec=ToyCodec(64), **kw)
    assert isinstance(coded.proj_in, torch.nn.Identity) and coded._cfg["Lc"] == 0
    coded.load_state_dict(plain.state_dict())
    plain, coded = plain.to(dev), coded.to(dev)
    wave = torch.randn(2, 640, generator=torch.Generator().manual_seed(1))
    lat = ToyCodec(64).encode(wave)
    gen = torch.Generator().manual_seed(2)
    draws = dict(x0=torch.randn(lat.shape, generator=gen), times=torch.rand(2, generator=gen), frac_lengths=torch.tensor([0.8, 0.9]),
                 rand=torch.rand(2, generator=gen))
    y0 = torch.randn(lat.shape, generator=gen)
    res = []
    for vb, inp in ((plain, lat), (coded, wave)):
        wr = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
        with rng_override(**draws):
            loss = wr(inp.to(dev))
        loss.backward()
        with rng_override(y0=y0):
            s = wr.sample(cond=inp.to(dev), steps=4, decode_to_audio=False)
        res.append((loss.detach(), [p.grad.clone() for p in vb.parameters() if p.grad is not None], s))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    assert len(res[0][1]) == len(res[1][1]) and all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))


def test_precise_mode_names_the_gap(golden):
    import voicebox_pytorch_amd as vbx

    g = golden("small_codec")
    vb = _build(g).eval()
    with vbx.precise_mode(), pytest.raises(NotImplementedError, match="precise mode"):
        vb(g["lat1"].to(dev), times=torch.tensor(0.5), cond_token_ids=None, cond=g["lat1"].to(dev), cond_drop_prob=0.0)
