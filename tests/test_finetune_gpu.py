"""GPU: fine-tuning on the device -- frozen parameters in dp.TrainStep, the LoRA kernels (csrc/lora.hip) against the fp64 restatement
tests/lora_ref.py with the bounds of include/vbx.h, and the adapter life cycle (add, train, save / load, merge, detach).
Model: dim 64 / depth 2 / heads 2, batches of 2 x 24 frames.  Every measured bound ratio is printed (profiles/finetune_parity.txt)."""
import pytest
import torch

import lora_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPES = [(64, 64, 1), (192, 64, 3), (340, 64, 8), (64, 170, 64)]  # r = 1, r % 4 != 0, the largest rank; K / N no multiples of 64
B_, N_, D_ = 2, 24, 64


def _model(seed=0, perturb=True):
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(seed)
    vb = vbx.VoiceBox(dim=D_, depth=2, heads=2, dim_head=64, condition_on_text=False)
    if perturb:  # the reference zero-initialises the adaLN projections: move them, so that their gradients and updates are not trivial
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():
            for n, p in vb.named_parameters():
                if ".to_gamma." in n or ".to_beta." in n:
                    p.add_(0.05 * torch.randn(p.shape, generator=g))
    vb = vb.to(dev)
    return vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def _draws(seed):
    g = torch.Generator().manual_seed(seed)
    return dict(x1=torch.randn(B_, N_, D_, generator=g), x0=torch.randn(B_, N_, D_, generator=g), times=torch.rand(B_, generator=g),
                frac_lengths=0.7 + 0.3 * torch.rand(B_, generator=g), rand=torch.rand(B_, generator=g))


def _step(ts, d, how="step", **kw):
    from voicebox_pytorch_amd.masks import rng_override

    with rng_override(**{k: v for k, v in d.items() if k != "x1"}):
        return getattr(ts, how)(d["x1"].to(dev), **kw)


def _sample(w, seed=3, steps=5):
    from voicebox_pytorch_amd.masks import rng_override

    g = torch.Generator().manual_seed(seed)
    cond, y0 = torch.randn(B_, N_, D_, generator=g), torch.randn(B_, N_, D_, generator=g)
    with rng_override(y0=y0):
        return w.sample(cond=cond.to(dev), steps=steps).clone()


def _eval_loss(w, d):
    from voicebox_pytorch_amd.masks import rng_override

    w.eval()
    with torch.inference_mode(), rng_override(**{k: v for k, v in d.items() if k != "x1"}):
        return float(w(d["x1"].to(dev)))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _ratio(got, want, bound):
    """largest |got - want| / bound over the elements (0 / 0 counts as 0)"""
    err = (got.double().cpu() - want).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


# ------------------------------------------------------------------------------------------- the kernels alone
def _rows(shapes, scale_of=lambda r: 8.0 / r):
    rows, w, l = [], 0, 0
    for N, K, r in shapes:
        a = l
        b = a + (r * K + 63) // 64 * 64
        l = b + (N * r + 63) // 64 * 64
        rows.append((w, w, a, b, N, K, r, scale_of(r)))
        w += (N * K + 63) // 64 * 64
    return rows, w, l


def _fill(rows, wn, ln, seed):
    g = torch.Generator().manual_seed(seed)
    w0, lflat, dW = torch.zeros(wn), torch.zeros(ln), torch.zeros(wn)
    for (wo, _, a, b, N, K, r, _) in rows:
        w0[wo:wo + N * K] = torch.randn(N * K, generator=g)
        dW[wo:wo + N * K] = torch.randn(N * K, generator=g)
        lflat[a:a + r * K] = torch.randn(r * K, generator=g) / K ** 0.5
        lflat[b:b + N * r] = torch.randn(N * r, generator=g)
    return w0, lflat, dW


@pytest.mark.parametrize("N,K,r", SHAPES)
def test_lora_apply_meets_its_bound(N, K, r):
    from voicebox_pytorch_amd.lora import LoraTable

    rows, wn, ln = _rows([(N, K, r)])
    w0, lflat, _ = _fill(rows, wn, ln, 11)
    w0[5] = -0.0
    tab = LoraTable(rows, wn, wn, ln)
    flat = torch.full((wn,), 7.0, device=dev)
    tab.apply(flat, w0.to(dev), lflat.to(dev))
    got = flat[:N * K].view(N, K).clone()
    A, Bm = lflat[:r * K].view(r, K), lflat[rows[0][3]:rows[0][3] + N * r].view(N, r)
    want, term = lora_ref.merge(w0[:N * K].view(N, K), A, Bm, 8.0)
    ratio = _ratio(got, want, lora_ref.merge_bound(term, r))
    rel = float((got.double().cpu() - want).abs().max() / want.abs().max())
    print(f"vbx_lora_apply ({N}, {K}, {r}): error / bound {ratio:.3f}, relative error {rel:.2e}")
    assert ratio <= 1.0 and rel < lora_ref.fault_tolerance()
    assert bool((flat[N * K:] == 7.0).all())  # nothing past the matrix is written
    again = torch.zeros(wn, device=dev)
    tab.apply(again, w0.to(dev), lflat.to(dev))
    assert torch.equal(_bits(again[:N * K]), _bits(flat[:N * K]))  # reruns are bit-identical
    lflat[rows[0][3]:] = 0.0  # B = 0: the bits of W0, its negative zero included
    tab.apply(again, w0.to(dev), lflat.to(dev))
    assert torch.equal(_bits(again[:N * K]).cpu(), _bits(w0[:N * K]))


def test_lora_grad_meets_its_bounds_alone_and_grouped():
    """The four shapes in ONE table (the table's largest rank picks the kernel), each against the restatement from the same dW; then
    each shape in a table of its own: bit-equal to its rows of the grouped run; reruns bit-identical."""
    from voicebox_pytorch_amd.lora import LoraTable

    rows, wn, ln = _rows(SHAPES)
    w0, lflat, dW = _fill(rows, wn, ln, 12)
    tab = LoraTable(rows, wn, wn, ln)
    gl = torch.full((ln,), 7.0, device=dev)
    scratch = torch.zeros(tab.scratch_floats, device=dev)
    tab.grad(dW.to(dev), lflat.to(dev), gl, scratch)
    gl2 = torch.zeros(ln, device=dev)
    tab.grad(dW.to(dev), lflat.to(dev), gl2, torch.ones(tab.scratch_floats, device=dev))
    tol = lora_ref.fault_tolerance()
    for (wo, _, a, b, N, K, r, s) in rows:
        A, Bm, G = lflat[a:a + r * K].view(r, K), lflat[b:b + N * r].view(N, r), dW[wo:wo + N * K].view(N, K)
        dA, dB, ta, tb = lora_ref.grads(G, A, Bm, 8.0)
        ba, bb = lora_ref.grad_bounds(ta, tb, N, K)
        gA, gB = gl[a:a + r * K].view(r, K), gl[b:b + N * r].view(N, r)
        ra, rb = _ratio(gA, dA, ba), _ratio(gB, dB, bb)
        print(f"vbx_lora_grad ({N}, {K}, {r}): dA error / bound {ra:.3f}, dB error / bound {rb:.3f}")
        assert ra <= 1.0 and rb <= 1.0
        assert float((gA.double().cpu() - dA).abs().max() / dA.abs().max()) < tol and float((gB.double().cpu() - dB).abs().max() / dB.abs().max()) < tol
        assert torch.equal(_bits(gA), _bits(gl2[a:a + r * K].view(r, K))) and torch.equal(_bits(gB), _bits(gl2[b:b + N * r].view(N, r)))
        # the same matrix in a table of its own (its own kernel instance when its rank is smaller than the table's largest)
        one, wn1, ln1 = _rows([(N, K, r)])
        t1 = LoraTable(one, wn1, wn1, ln1)
        l1 = torch.zeros(ln1)
        l1[:r * K], l1[one[0][3]:one[0][3] + N * r] = A.reshape(-1), Bm.reshape(-1)
        g1 = torch.zeros(ln1, device=dev)
        t1.grad(G.reshape(-1).contiguous().to(dev), l1.to(dev), g1, torch.zeros(max(1, t1.scratch_floats), device=dev))
        assert torch.equal(_bits(g1[:r * K]), _bits(gA).reshape(-1)) and torch.equal(_bits(g1[one[0][3]:one[0][3] + N * r]), _bits(gB).reshape(-1))
    pad = torch.ones(ln, dtype=torch.bool)
    for (_, _, a, b, N, K, r, _) in rows:
        pad[a:a + r * K] = False
        pad[b:b + N * r] = False
    assert bool((gl.cpu()[pad] == 7.0).all())  # the padding between the adapters is not written


# ------------------------------------------------------------------------------------------- frozen parameters
def _freeze_three(vb):
    frozen = [vb.transformer.layers[0][3].to_qkv.weight, vb.transformer.layers[1][4].to_beta.weight, vb.to_pred.weight]
    for p in frozen:
        p.requires_grad_(False)
    return frozen


def _range_of(fp, p):
    s = next(s for s in fp.order if fp.slots[s] is p)
    return fp.offsets[s], fp.offsets[s] + p.numel()


def test_frozen_tensors_do_not_move():
    """to_qkv.weight of layer 0, one adaLN weight and to_pred frozen, three steps: their bits and their m / v stay; with
    max_grad_norm=None and identical draws every other tensor is bit-equal to an unfrozen TrainStep in the adaLN mode the frozen
    step resolves to (one adaLN weight frozen: mixed -> "materialize") and whose three tensors are put back after each of its steps."""
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(1)
    start = vb.flat_params().flat.clone()
    frozen = _freeze_three(vb)
    ts = TrainStep(w, lr=1e-3, max_grad_norm=None)
    assert ts._filter["adaln"] == "mixed" and not ts.adaln_factors_apply(batch=B_)
    vb2, w2 = _model(1)
    ts2 = TrainStep(w2, lr=1e-3, max_grad_norm=None, adaln_grads="materialize")
    assert torch.equal(vb2.flat_params().flat, start)
    fp, flat, flat2 = ts.fp, ts.fp.flat, ts2.fp.flat
    where = [_range_of(fp, p) for p in frozen]
    for i in range(3):
        _step(ts, _draws(20 + i))
        _step(ts2, _draws(20 + i))
        for lo, hi in where:
            # the unfrozen step does move these tensors; they are put back, so that its next step differentiates the same function
            # (Adam is elementwise: the other tensors and their moments then follow the frozen run's trajectory exactly)
            assert not torch.equal(flat2[lo:hi], start[lo:hi])
            flat2[lo:hi].copy_(start[lo:hi])
    torch.cuda.synchronize()
    moved = torch.zeros(fp.numel, dtype=torch.bool, device=dev)
    for lo, hi in where:
        assert torch.equal(_bits(flat[lo:hi]), _bits(start[lo:hi])), "a frozen tensor changed"
        assert float(ts.m[lo:hi].abs().max()) == 0.0 and float(ts.v[lo:hi].abs().max()) == 0.0
        moved[lo:hi] = True
    assert torch.equal(_bits(flat[~moved]), _bits(flat2[~moved])), "a trainable tensor differs from the unfrozen step"
    assert torch.equal(_bits(ts.m[~moved]), _bits(ts2.m[~moved])) and torch.equal(_bits(ts.v[~moved]), _bits(ts2.v[~moved]))
    assert not torch.equal(flat[~moved], start[~moved])
    # the frozen step's training engine kept operand copies that match its master weights (the filtered Adam refreshes what it
    # updates, the rest never changed): its next loss equals the first loss of a fresh model holding the same weights
    vb3, w3 = _model(1)
    vb3.flat_params().flat.copy_(flat)
    l4 = float(_step(ts, _draws(30)))
    assert l4 == float(_step(TrainStep(w3, lr=1e-3, max_grad_norm=None), _draws(30)))


@pytest.mark.parametrize("case", ["mixed", "adaln_frozen", "adaln_trainable"])
def test_clip_norm_over_the_trainable_gradients(case):
    """clipping on: coef[1] against the fp64 norm of the trainable gradients (the relative 2e-6 of
    test_gradient_norm_from_slab_reduce_partials), in the three adaLN modes; frozen tensors keep their bits."""
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(2)
    frozen = [vb.transformer.layers[0][3].to_qkv.weight, vb.to_pred.weight, vb.transformer.layers[1][5][0].bias]
    if case == "mixed":
        frozen.append(vb.transformer.layers[1][4].to_beta.weight)
    if case == "adaln_frozen":
        frozen += [m.weight for l in range(2) for i in (2, 4) for m in (vb.transformer.layers[l][i].to_gamma, vb.transformer.layers[l][i].to_beta)]
    for p in frozen:
        p.requires_grad_(False)
    ts = TrainStep(w, lr=1e-3, max_grad_norm=0.5)
    assert ts._filter["adaln"] == {"mixed": "mixed", "adaln_frozen": "none", "adaln_trainable": "all"}[case]
    assert ts.adaln_factors_apply(batch=B_) == (case != "mixed")
    start = ts.fp.flat.clone()
    _step(ts, _draws(40))
    torch.cuda.synchronize()
    fp = ts.fp
    # the reference gradient: the same weights and draws with everything trainable and materialised
    vb2, w2 = _model(2)
    ts2 = TrainStep(w2, lr=1e-3, max_grad_norm=0.5, adaln_grads="materialize")
    _step(ts2, _draws(40))
    g = ts2.gflat.double().cpu()
    keep = torch.ones(fp.numel, dtype=torch.bool)
    for p in frozen:
        lo, hi = _range_of(fp, p)
        keep[lo:hi] = False
        assert torch.equal(_bits(fp.flat[lo:hi]), _bits(start[lo:hi]))
    want = float(g[keep].norm())
    got = float(ts.coef[1])
    print(f"clip norm ({case}): {got:.8e} against fp64 {want:.8e}, relative {abs(got - want) / want:.2e}")
    assert abs(got - want) < 2e-6 * want
    assert want < float(g.norm()) * (1 - 1e-4)  # (the frozen tensors' share is not negligible: the check can tell)
    assert not torch.equal(fp.flat[keep.to(dev)], start[keep.to(dev)])


def test_accumulation_leaves_frozen_tensors_alone():
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(3)
    frozen = _freeze_three(vb)
    ts = TrainStep(w, lr=1e-3, max_grad_norm=0.5)
    start = ts.fp.flat.clone()
    _step(ts, _draws(50), "accumulate", weight=0.5)
    _step(ts, _draws(51), "accumulate", weight=0.5)
    ts.apply_accumulated()
    _step(ts, _draws(52), "accumulate", weight=0.5)
    _step(ts, _draws(53), "accumulate_last_and_apply", weight=0.5)
    torch.cuda.synchronize()
    for p in frozen:
        lo, hi = _range_of(ts.fp, p)
        assert torch.equal(_bits(ts.fp.flat[lo:hi]), _bits(start[lo:hi])) and float(ts.m[lo:hi].abs().max()) == 0.0
    assert not torch.equal(ts.fp.flat, start)


# ------------------------------------------------------------------------------------------- adapters on the model
def test_add_lora_changes_no_bit():
    """Right after add_lora (B = 0): the master weights, the loss of a fixed batch and a 4-interval sample are bit-equal to the plain
    model's; refusals on the GPU model raise before any launch."""
    import voicebox_pytorch_amd as vbx

    vb, w = _model(4)
    flat0 = vb.flat_params().flat.clone()
    loss0, s0 = _eval_loss(w, _draws(60)), _sample(w)
    vb.add_lora(rank=3, alpha=6.)
    assert torch.equal(_bits(vb.flat_params().flat), _bits(flat0))
    assert _eval_loss(w, _draws(60)) == loss0 and torch.equal(_bits(_sample(w)), _bits(s0))
    vb._lora.needs_apply = True  # the merge kernel itself with B = 0: still no bit
    vb._lora.apply()
    torch.cuda.synchronize()
    assert torch.equal(_bits(vb.flat_params().flat), _bits(flat0))
    with pytest.raises(NotImplementedError, match="TrainStep"):
        w(_draws(60)["x1"].to(dev))
    with vbx.precise_mode():
        with pytest.raises(NotImplementedError):
            vb.engine(B_, N_, training=False)
    with pytest.raises(ValueError):
        vb.add_lora()


def _random_b(vb, seed):
    g = torch.Generator().manual_seed(seed)
    sd = vb.lora_state_dict()
    vb.load_lora_state_dict({k: (0.05 * torch.randn(v.shape, generator=g) if k.endswith("lora_B") else v) for k, v in sd.items()})


def _adapter_grad_ratios(ts, tag):
    """every adapter's gradient in the step's buffer against the restatement from the dW in the step's own gradient buffer"""
    st, lo, fp = ts.vb._lora, ts._lora_rt, ts.fp
    worst = 0.0
    for e in st.entries:
        N, K, r = e["N"], e["K"], st.rank
        o = fp.offsets[e["slot"]]
        dW = ts.gflat[o:o + N * K].view(N, K).cpu()
        A, Bm = e["module"].lora_A.detach().cpu(), e["module"].lora_B.detach().cpu()
        dA, dB, ta, tb = lora_ref.grads(dW, A, Bm, st.alpha)
        ba, bb = lora_ref.grad_bounds(ta, tb, N, K)
        ra = _ratio(lo["g"][e["a_off"]:e["a_off"] + r * K].view(r, K), dA, ba)
        rb = _ratio(lo["g"][e["b_off"]:e["b_off"] + N * r].view(N, r), dB, bb)
        worst = max(worst, ra, rb)
    print(f"adapter gradients in the step ({tag}): largest error / bound {worst:.3f}")
    return worst


def test_adapter_gradients_in_the_step_and_under_accumulation():
    """Teacher-forced from the kernel's own dW: lr = 0 keeps A and B where the gradient was taken.  Then two accumulated micro-batches:
    the adapter gradients against the accumulated dW, frozen tensors untouched; and the merged weights against the restatement."""
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(5)
    vb.add_lora(rank=3, alpha=6.)
    _random_b(vb, 70)
    st = vb._lora
    for e in st.entries:  # vbx_lora_apply inside the model: W_eff against the restatement
        want, term = lora_ref.merge(st.w0_view(e).cpu(), e["module"].lora_A.detach().cpu(), e["module"].lora_B.detach().cpu(), st.alpha)
        assert _ratio(e["module"].weight.detach(), want, lora_ref.merge_bound(term, st.rank)) <= 1.0
        assert not torch.equal(e["module"].weight.detach(), st.w0_view(e))
    ts = TrainStep(w, lr=0.0, max_grad_norm=0.5)
    base = ts.fp.flat.clone()
    _step(ts, _draws(71))
    torch.cuda.synchronize()
    assert _adapter_grad_ratios(ts, "one step") <= 1.0
    gl = ts._lora_rt["g"].double().cpu()
    assert abs(float(ts.coef[1]) - float(gl.norm())) < 2e-6 * float(gl.norm())  # nothing but the adapters is trainable
    _step(ts, _draws(72), "accumulate", weight=0.5)
    _step(ts, _draws(73), "accumulate", weight=0.5)
    ts.apply_accumulated()
    torch.cuda.synchronize()
    assert _adapter_grad_ratios(ts, "two accumulated micro-batches") <= 1.0
    assert torch.equal(_bits(ts.fp.flat), _bits(base)) and float(ts.m.abs().max()) == 0.0  # lr = 0 and a frozen base: no bit moved


def test_clip_norm_with_adapters_and_a_trainable_base():
    """add_lora(train_base=True): the norm is taken in two launches (the trainable ranges of the base, then the adapter gradients, the
    first one's sum handed on through the scratch) plus the adaLN Gram terms of the factor form; against fp64 from the step's own
    buffers.  The adapted matrices' dW is in the gradient buffer but takes no part; every other tensor and the adapters move."""
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(11)
    vb.add_lora(rank=3, alpha=6., train_base=True)
    _random_b(vb, 12)
    ts = TrainStep(w, lr=1e-3, max_grad_norm=0.5)
    assert ts._filter["adaln"] == "all" and ts.adaln_factors_apply(batch=B_) and ts._filter["any_base"]
    st, fp = vb._lora, ts.fp
    start, w0, l0 = fp.flat.clone(), st.w0.clone(), st.lflat.clone()
    _step(ts, _draws(13))
    torch.cuda.synchronize()
    g = ts.gflat.double().cpu()
    dada, temb = ts._last_eng.adaln_factor_tensors()
    for l, (lo, hi) in enumerate(ts.adaln_weight_ranges()):  # the factor-form blocks, materialised on the host
        g[lo:hi] = (dada[l].double().t() @ temb.double()).reshape(-1).cpu()
    keep = torch.ones(fp.numel, dtype=torch.bool)
    for e in st.entries:
        o = fp.offsets[e["slot"]]
        keep[o:o + e["N"] * e["K"]] = False
        assert float(ts.gflat[o:o + e["N"] * e["K"]].abs().max()) > 0 and float(ts.m[o:o + e["N"] * e["K"]].abs().max()) == 0.0
    gl = ts._lora_rt["g"].double().cpu()
    want = float((g[keep].pow(2).sum() + gl.pow(2).sum()).sqrt())
    got = float(ts.coef[1])
    print(f"clip norm (adapters + trainable base, factor-form adaLN): {got:.8e} against fp64 {want:.8e}, relative {abs(got - want) / want:.2e}")
    assert abs(got - want) < 2e-6 * want and float(gl.norm()) > 1e-3 * want and float(g[keep].norm()) > 1e-3 * want
    assert torch.equal(_bits(st.w0), _bits(w0)) and not torch.equal(st.lflat, l0)
    assert not torch.equal(fp.flat[keep.to(dev)], start[keep.to(dev)])
    for e in st.entries:  # the master slot holds W0 + s.B.A of the UPDATED adapters
        want_w, term = lora_ref.merge(st.w0_view(e).cpu(), e["module"].lora_A.detach().cpu(), e["module"].lora_B.detach().cpu(), st.alpha)
        assert _ratio(e["module"].weight.detach(), want_w, lora_ref.merge_bound(term, st.rank)) <= 1.0


def test_twenty_adam_steps_then_merge_and_detach():
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(6)
    sd0 = {k: v.clone() for k, v in vb.state_dict().items()}
    vb.add_lora(rank=8, alpha=16.)
    d = _draws(80)
    s_before = _sample(w)  # captures the sampler's graph on the un-trained adapters
    ts = TrainStep(w, lr=2e-3, max_grad_norm=0.5)
    first = float(_step(ts, d))
    for _ in range(19):
        last = float(_step(ts, d))
    print(f"twenty LoRA steps on a fixed batch: loss {first:.5f} -> {last:.5f}")
    assert last < first
    sd = vb.state_dict()
    assert all(torch.equal(_bits(sd[k]), _bits(sd0[k])) for k in sd0), "a base tensor changed"  # W0 and every un-adapted tensor
    lsd = vb.lora_state_dict()
    assert all(float(v.abs().max()) > 0 for v in lsd.values())
    adapted = {e["key"] for e in vb._lora.entries}
    live = dict(vb.named_parameters())
    assert all(torch.equal(_bits(live[k]), _bits(sd0[k])) == (k not in adapted) for k in sd0 if k in live)
    # the sampler captured before the steps serves the new weights: bit-equal to a fresh wrapper over the same model
    import voicebox_pytorch_amd as vbx

    s_att = _sample(w)
    assert not torch.equal(s_att, s_before)
    assert torch.equal(_bits(s_att), _bits(_sample(vbx.ConditionalFlowMatcherWrapper(voicebox=vb))))
    # detach restores every base tensor bit for bit; attaching the saved adapters again gives the same model
    w_eff = {e["key"]: e["module"].weight.detach().clone() for e in vb._lora.entries}
    vb.detach_lora()
    sd1 = vb.state_dict()
    assert set(sd1) == set(sd0) and all(torch.equal(_bits(sd1[k]), _bits(sd0[k])) for k in sd0)
    assert torch.equal(_bits(_sample(w)), _bits(s_before))
    vb.add_lora(rank=8, alpha=16.)
    vb.load_lora_state_dict(lsd)
    assert all(torch.equal(_bits(live[k]), _bits(w_eff[k])) for k in w_eff)
    assert torch.equal(_bits(_sample(w)), _bits(s_att))
    # merge keeps W_eff in a plain model
    vb.merge_lora()
    assert set(vb.state_dict()) == set(sd0) and all(torch.equal(_bits(vb.state_dict()[k]), _bits(w_eff[k])) for k in w_eff)
    assert torch.equal(_bits(_sample(w)), _bits(s_att))
    assert all(p.requires_grad for n, p in vb.named_parameters() if n != "null_cond")


def test_state_dict_round_trips():
    vb, w = _model(7)
    vb.add_lora(rank=3, alpha=6., layers=[1])
    _random_b(vb, 90)
    sd, lsd, flat = {k: v.clone() for k, v in w.state_dict().items()}, vb.lora_state_dict(), vb.flat_params().flat.clone()
    vb2, w2 = _model(8)
    vb2.add_lora(rank=3, alpha=6., layers=[1])
    w2.load_state_dict(sd)  # W0 and the adapters, re-applied
    torch.cuda.synchronize()
    sd2 = w2.state_dict()
    assert set(sd2) == set(sd) and all(torch.equal(_bits(sd2[k]), _bits(sd[k])) for k in sd)
    assert torch.equal(_bits(vb2.flat_params().flat), _bits(flat))
    vb3, w3 = _model(7)
    vb3.add_lora(rank=3, alpha=6., layers=[1])
    vb3.load_lora_state_dict(lsd)
    assert torch.equal(_bits(vb3.flat_params().flat), _bits(flat))
    # a write through .data + mark_weights_dirty re-applies
    with torch.no_grad():
        vb3.transformer.layers[1][3].to_out.lora_B.data.zero_()
    vb3.mark_weights_dirty()
    assert torch.equal(_bits(vb3.transformer.layers[1][3].to_out.weight), _bits(vb3._lora.w0_view(vb3._lora.entries[1])))


class _Latents(torch.utils.data.Dataset):
    def __init__(self, n=8):
        g = torch.Generator().manual_seed(5)
        self.x = [torch.randn(N_, D_, generator=g) for _ in range(n)]

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i]


def test_trainer_save_load_round_trip(tmp_path):
    """VoiceBoxTrainer over an adapted wrapper: three steps, save, one more step -- against a second trainer that loads the checkpoint
    into a freshly adapted model and takes that step: the loss and the adapters are bit-equal to the uninterrupted run."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    def trainer(seed, folder):
        vb, w = _model(seed)
        vb.add_lora(rank=3, alpha=6.)
        return vb, vbx.VoiceBoxTrainer(w, batch_size=2, dataset=_Latents(), num_train_steps=10, lr=1e-3, valid_frac=0., log_every=1000,
                                       save_results_every=1000, save_model_every=1000, results_folder=str(folder), length_bucket=0)

    d = _draws(95)
    draws = {k: v for k, v in d.items() if k != "x1"}
    vb, tr = trainer(9, tmp_path / "a")
    batch = torch.stack(tr.ds.x[:2])
    for i in range(3):
        with rng_override(**draws):
            tr.train_step_fn.step(batch.to(dev), lr=1e-3)
    path = str(tmp_path / "voicebox.3.pt")
    tr.save(path)
    with rng_override(**draws):
        want = float(tr.train_step_fn.step(batch.to(dev), lr=1e-3))
    vb2, tr2 = trainer(10, tmp_path / "b")
    tr2.load(path)
    assert tr2.train_step_fn.steps == 3
    with rng_override(**draws):
        got = float(tr2.train_step_fn.step(batch.to(dev), lr=1e-3))
    assert got == want
    a, b = vb.lora_state_dict(), vb2.lora_state_dict()
    assert all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)
    assert torch.equal(_bits(vb.flat_params().flat), _bits(vb2.flat_params().flat))
    logs = tr2.train_step()  # the trainer's own step (data loader, schedule) runs over the adapted wrapper
    assert logs["loss"] == logs["loss"]
