"""The Aligner network on the device (csrc/aligner.hip, align.py) against tests/aligner_ref.py in fp64.

aligner_attention is held to the bounds of include/vbx.h teacher-forced (the reference sees the kernel's own fp32 operands); the
module, whose GEMM operands are fp16 (forward; an fp16 hi + lo pair in front of a ReLU) and bf16 (backward), to the tolerance that
tests/test_aligner_cpu.py derives from the planted faults of the restatement (aligner_ref.tolerance(), a tenth of the smallest
planted movement: 0.0222), against the fp64 restatement and against the same with the forward's operand roundings emulated.

`pytest -s -m gpu tests/test_aligner_gpu.py` prints the lines kept in profiles/aligner_parity.txt."""
import functools

import pytest
import torch

import aligner_ref as R

import voicebox_pytorch_amd as vbx

pytestmark = pytest.mark.gpu

TAU = 0.0005
TAU32 = float(torch.tensor(TAU, dtype=torch.float32))  # what the kernels are handed
# (dim_in, dim_hidden, attn_channels), B, T, K: the tile tails, the 80-channel tail, the 3-tap edges at T = 1 and 2, the key limit
CASES = [((80, 64, 80), 3, 1, 1), ((80, 64, 80), 3, 2, 3), ((80, 64, 80), 2, 5, 1), ((80, 64, 80), 2, 67, 65),
         ((80, 64, 80), 2, 130, 200), ((80, 512, 80), 2, 67, 65), ((16, 64, 8), 3, 33, 17), ((128, 128, 128), 1, 1032, 1024)]
IDS = [f"{d[0]}-{d[1]}-{d[2]}_{B}x{T}x{K}" for d, B, T, K in CASES]
RECORD = {}


def _note(key, value):
    RECORD[key] = max(RECORD.get(key, 0.0), float(value))


def _module(dims, sd):
    m = vbx.Aligner(dim_in=dims[0], dim_hidden=dims[1], attn_channels=dims[2], temperature=TAU).cuda()
    m.load_state_dict(sd)
    return m


def _bin_term(attn, path):
    return -(torch.log(attn.clamp(min=1e-12)) * path).sum() / path.sum().clamp(min=1)


def _device_run(mod, queries, keys, klens, qlens):
    """one forward + backward of the module under the forward-sum loss plus the binarisation term: everything on the host"""
    T, K = queries.shape[2], keys.shape[1]
    dev = "cuda"
    q, k = queries.to(dev).requires_grad_(), keys.to(dev).requires_grad_()
    kl, ql = torch.tensor(klens, device=dev), torch.tensor(qlens, device=dev)
    for p in mod.parameters():
        p.grad = None
    attn, lp = mod(q, k, R.mask_of(klens, K).to(dev))
    loss = vbx.ForwardSumLoss()(lp, kl, ql) + _bin_term(attn, R.planted_path(klens, qlens, T, K).float().to(dev))
    loss.backward()
    grads = {n: p.grad.detach().cpu() for n, p in mod.named_parameters()}
    grads.update(queries=q.grad.cpu(), keys=k.grad.cpu())
    return dict(attn=attn.detach().cpu(), logprob=lp.detach().cpu(), loss=float(loss.detach()), grads=grads)


@functools.lru_cache(maxsize=None)
def _case(i, variant):
    dims, B, T, K = CASES[i]
    sd = R.init_state(*dims, seed=i + 1, tau=TAU)
    queries, keys = R.make_inputs(B, T, K, dims[0], dims[1], seed=100 + i)
    klens, qlens = R.lengths(B, T, K, variant)
    mask = R.mask_of(klens, K)
    mod = _module(dims, sd)
    out = _device_run(mod, queries, keys, klens, qlens)
    ref = R.reference(sd, queries, keys, klens, qlens, TAU)
    with torch.no_grad():
        emu = R.forward(sd, queries, keys, mask, TAU, emulate=True)
        q64, k64, _ = R.encode(sd, queries.double(), keys.double())
    return dict(dims=dims, sd=sd, queries=queries, keys=keys, klens=klens, qlens=qlens, mask=mask, mod=mod, out=out, ref=ref, emu=emu,
                q32=q64.float(), k32=k64.float())


def _variants(i):
    return R.variants(CASES[i][1])


# ----------------------------------------------------------------------------- the attention op, teacher-forced
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_attention_forward_meets_its_bounds(i):
    A = CASES[i][0][2]
    for v in _variants(i):
        c = _case(i, v)
        q, k, mask = c["q32"], c["k32"], c["mask"]
        attn, lp = vbx.aligner_attention(q.cuda(), k.cuda(), mask.cuda(), TAU)
        attn, lp = attn.cpu(), lp.cpu()
        assert attn.dtype == lp.dtype == torch.float32 and attn.shape == lp.shape == (q.shape[0], 1, q.shape[1], k.shape[1])
        ref = R.attention(q.double(), k.double(), None, TAU32)[1]
        err, bound = (lp.double() - ref).abs(), R.logprob_bound(ref, A)
        assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
        _note("attention forward: |attn_logprob - fp64| / ((A + 4) u |ref|)", (err / bound.clamp(min=1e-300)).max())
        _note("attention forward: attn_logprob error, units of 2^-24 |ref|", (err / (R.U24 * ref.abs()).clamp(min=1e-300)).max())
        p, pb = R.softmax_ref_and_bound(lp, mask)
        perr = (attn.double() - p).abs()
        assert bool((perr <= pb).all()), float((perr / pb).max())
        _note("attention forward: |attn - fp64 softmax of own logprob| / bound", (perr / pb).max())
        live = mask.any(1)
        gone = (~mask[:, None, None, :]).expand_as(attn) & live[:, None, None, None]
        assert float(attn[gone].abs().sum()) == 0.0  # a masked key: exactly 0
        if bool((~live).any()):  # a fully masked row: exactly 1 / K
            assert torch.equal(attn[~live], torch.full_like(attn[~live], 1.0) / k.shape[1])
        # no mask at all = a mask of ones, bit for bit; a second run gives the same bits
        a2, l2 = vbx.aligner_attention(q.cuda(), k.cuda(), mask.cuda(), TAU)
        assert torch.equal(a2.cpu(), attn) and torch.equal(l2.cpu(), lp)
        a3, l3 = vbx.aligner_attention(q.cuda(), k.cuda(), None, TAU)
        a4, l4 = vbx.aligner_attention(q.cuda(), k.cuda(), torch.ones_like(mask, dtype=torch.int32).cuda()[:, None], TAU)
        assert torch.equal(a3, a4) and torch.equal(l3, l4) and torch.equal(l3.cpu(), lp)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_attention_backward_meets_its_bounds(i):
    for v in _variants(i):
        c = _case(i, v)
        q, k, mask = c["q32"], c["k32"], c["mask"]
        B, T, A = q.shape
        K = k.shape[1]
        g = torch.Generator().manual_seed(7 + i)
        ga, gl = torch.randn(B, 1, T, K, generator=g), torch.randn(B, 1, T, K, generator=g)
        for name, use_a, use_l in (("g_logprob", False, True), ("g_attn", True, False), ("both", True, True)):
            qd, kd = q.cuda().requires_grad_(), k.cuda().requires_grad_()
            attn, lp = vbx.aligner_attention(qd, kd, mask.cuda(), TAU)
            outs = [t for t, u in ((attn, use_a), (lp, use_l)) if u]
            gs = [t.cuda() for t, u in ((ga, use_a), (gl, use_l)) if u]
            dq, dk = torch.autograd.grad(outs, (qd, kd), gs)
            dq2, dk2 = torch.autograd.grad(vbx.aligner_attention(qd, kd, mask.cuda(), TAU)[1 - use_a:1 + use_l], (qd, kd), gs)
            assert torch.equal(dq, dq2) and torch.equal(dk, dk2)  # reruns: the same bits
            own = attn.detach().cpu()
            rq, rk, _ = R.attention_backward(q.double(), k.double(), mask, TAU32, own.double(), ga.double() if use_a else None,
                                             gl.double() if use_l else None)
            bq, bk = R.attn_grad_bounds(q, k, mask, TAU32, own, ga if use_a else None, gl if use_l else None)
            for what, d, r, b in (("dq", dq, rq, bq), ("dk", dk, rk, bk)):
                err = (d.cpu().double() - r).abs()
                assert bool((err <= b).all()), (name, what, float((err / b.clamp(min=1e-300)).max()))
                _note(f"attention backward from {name}: |{what} - fp64| / bound", (err / b.clamp(min=1e-300)).max())
            # one gradient alone: the same bits as beside the other
            dq3, = torch.autograd.grad(vbx.aligner_attention(qd, k.cuda(), mask.cuda(), TAU)[1 - use_a:1 + use_l], (qd,), gs)
            assert torch.equal(dq3, dq)


# ----------------------------------------------------------------------------- the module
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_module_forward_within_the_tolerance(i):
    tol = R.tolerance()
    for v in _variants(i):
        c = _case(i, v)
        out, ref, (ea, el) = c["out"], c["ref"], c["emu"]
        assert out["attn"].shape == ref["attn"].shape and out["logprob"].dtype == torch.float32
        for name, a, l in (("fp64", ref["attn"], ref["logprob"]), ("emulated operands", ea, el)):
            ml, ma = R.logprob_movement(out["logprob"], l), float((out["attn"].double() - a).abs().max())
            print(f"{IDS[i]} variant {v}: attn_logprob max |err| / RMS {ml:.3e}, attn max |err| {ma:.3e} against {name}")
            _note(f"module forward: attn_logprob max |err| / RMS against {name}", ml)
            _note(f"module forward: attn max |err| against {name}", ma)
            assert ml <= tol and ma <= tol, (name, ml, ma, tol)
        live = c["mask"].any(1)
        gone = (~c["mask"][:, None, None, :]).expand_as(out["attn"]) & live[:, None, None, None]
        assert float(out["attn"][gone].abs().sum()) == 0.0
        if CASES[i][3] > 1:  # the trained regime: the map is not flat
            spread = float(ref["logprob"].std(3).mean())
            assert 0.5 < spread < 6.0, spread


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_module_gradients_within_the_tolerance(i):
    tol = R.tolerance()
    for v in _variants(i):
        c = _case(i, v)
        out, ref = c["out"], c["ref"]
        assert abs(out["loss"] - float(ref["loss"])) <= tol * max(1.0, abs(float(ref["loss"])))
        assert set(out["grads"]) == set(ref["grads"])
        for n, r in ref["grads"].items():
            g = out["grads"][n]
            assert g.shape == r.shape and g.dtype == torch.float32, n
            e = R.rel_l2(g, r)
            if float(r.norm()) == 0.0:  # e.g. every row without a path: nothing flows, exactly
                assert float(g.abs().max()) == 0.0, n
                continue
            print(f"{IDS[i]} variant {v}: {n} relative L2 {e:.3e}")
            _note("module backward: largest relative L2 of a gradient tensor against the fp64 autograd", e)
            assert e <= tol, (n, e, tol)


@pytest.mark.parametrize("i", [1, 3, 6], ids=[IDS[1], IDS[3], IDS[6]])
def test_module_reruns_and_rows_are_bit_equal(i):
    c = _case(i, 0)
    again = _device_run(c["mod"], c["queries"], c["keys"], c["klens"], c["qlens"])
    assert torch.equal(again["attn"], c["out"]["attn"]) and torch.equal(again["logprob"], c["out"]["logprob"])
    for n, g in c["out"]["grads"].items():
        assert torch.equal(again["grads"][n], g), n
    with torch.no_grad():
        for b in range(c["queries"].shape[0]):  # a row alone: the bits it has in the batch
            a, l = c["mod"](c["queries"][b:b + 1].cuda(), c["keys"][b:b + 1].cuda(), c["mask"][b:b + 1].cuda())
            assert torch.equal(a.cpu(), c["out"]["attn"][b:b + 1]) and torch.equal(l.cpu(), c["out"]["logprob"][b:b + 1])
        # the mel as a transposed [B, T, dim_in] tensor (what forward_aligner passes) is read in place: the same bits
        rows = c["queries"].transpose(1, 2).contiguous().cuda()
        a, l = c["mod"](rows.transpose(1, 2), c["keys"].cuda(), c["mask"].cuda())
        assert torch.equal(a.cpu(), c["out"]["attn"]) and torch.equal(l.cpu(), c["out"]["logprob"])


def test_weights_are_repacked_per_parameter_version():
    c = _case(6, 0)
    mod = _module(c["dims"], c["sd"])
    q, k = c["queries"].cuda(), c["keys"].cuda()
    with torch.no_grad():
        l0 = mod(q, k)[1]
        mod.key_layers[2].weight *= 2.0  # an in-place update moves the version counter
        l1 = mod(q, k)[1]
        assert not torch.equal(l0, l1)
        mod.key_layers[2].weight.data *= 0.5  # a write through .data does not ...
        assert torch.equal(mod(q, k)[1], l1)
        mod.mark_weights_dirty()  # ... until the caller says so
        assert torch.equal(mod(q, k)[1], l0)


def _small_dp(seed=3):
    dp = vbx.DurationPredictor(num_phoneme_tokens=12, dim_phoneme_emb=64, dim=64, depth=2, dim_head=64, heads=2,
                               aligner_kwargs=dict(dim_in=80, attn_channels=80)).cuda()
    dp.attach_aligner()
    dp.aligner.load_state_dict(R.init_state(80, 64, 80, seed, TAU))
    return dp.eval()


def test_no_host_synchronisation():
    c = _case(3, 0)
    dp = _small_dp()
    q, k, mask = c["queries"].cuda().requires_grad_(), c["keys"].cuda().requires_grad_(), c["mask"].cuda()
    kl, ql = torch.tensor(c["klens"], device="cuda"), torch.tensor(c["qlens"], device="cuda")
    ymask = (torch.arange(q.shape[2], device="cuda")[None] < ql[:, None])[:, None]
    fsl = vbx.ForwardSumLoss()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        attn, lp = c["mod"](q, k, mask)
        (fsl(lp, kl, ql) + attn.square().sum()).backward()
        c["mod"].align(q.detach(), k.detach(), kl, ql)
        dp.forward_aligner(k.detach(), mask[:, None], q.detach().transpose(1, 2), ymask)
        a, l = vbx.aligner_attention(attn[:, 0].detach().requires_grad_(), attn[:, 0].detach(), None, TAU)
        (a.sum() + l.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- wiring
def _repeat_ids(ids, durations):
    """align_phoneme_ids_with_durations restated: id i repeated max(d_i, 1) times, zeros up to the longest row"""
    rows = [torch.repeat_interleave(i, d.clamp(min=1)) for i, d in zip(ids, durations)]
    n = max(len(r) for r in rows)
    return torch.stack([torch.cat((r, r.new_zeros(n - len(r)))) for r in rows])


def test_duration_predictor_wiring():
    dp = _small_dp()
    g = torch.Generator().manual_seed(9)
    B, Tx, Ty = 3, 17, 67
    ids = torch.randint(0, 12, (B, Tx), generator=g)
    klens, qlens = [17, 11, 0], [67, 54, 67]
    ids[1, 11:] = -1
    ids[2, :] = -1
    x_mask, y_mask = R.mask_of(klens, Tx)[:, None].cuda(), R.mask_of(qlens, Ty)[:, None].cuda()
    mel = torch.randn(B, Ty, 80, generator=g).cuda()
    with torch.no_grad():
        x = dp.to_phoneme_emb(ids.clamp(min=0).cuda())
        hard, soft, logprob, mas = dp.forward_aligner(x, x_mask.int(), mel, y_mask.int())
        assert hard.shape == (B, Tx) and hard.dtype == torch.float32 and soft.shape == mas.shape == (B, Tx, Ty)
        assert logprob.shape == (B, 1, Ty, Tx)
        assert soft.transpose(1, 2).is_contiguous() and mas.transpose(1, 2).is_contiguous()  # transposed views, no copy
        a, l = dp.aligner(mel.transpose(1, 2), x, x_mask)
        assert torch.equal(a[:, 0].transpose(1, 2), soft) and torch.equal(l, logprob)
        # the hard alignment is maximum_path on the module's OWN soft map (a path against fp64 would hang on ties)
        kl, ql = torch.tensor(klens, device="cuda"), torch.tensor(qlens, device="cuda")
        path, dur = vbx.maximum_path(soft.transpose(1, 2).contiguous(), ql, kl)
        assert torch.equal(path.transpose(1, 2), mas) and torch.equal(dur.float(), hard)
        d2, p2 = dp.aligner.align(mel.transpose(1, 2), x, key_lens=kl, query_lens=ql)
        assert torch.equal(d2, dur) and torch.equal(p2[:, 0], path) and d2.dtype == torch.int64
        assert dur.sum(1).tolist() == [67, 54, 0]  # feasible rows: every live frame on one key
        aligned = dp.align_phoneme_ids(mel.transpose(1, 2), ids.cuda(), mel_len=ql)
        assert torch.equal(aligned.cpu(), _repeat_ids(ids.clamp(min=0), dur.cpu()))
        assert torch.equal(dp.align_phoneme_ids(mel.transpose(1, 2), ids.cuda(), phoneme_len=kl, mel_len=ql), aligned)
    # the aligner's parameters train through forward_aligner's differentiable outputs
    _, soft, logprob, _ = dp.forward_aligner(x, x_mask, mel, y_mask)
    (vbx.ForwardSumLoss()(logprob, kl, ql) + soft.square().mean()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in dp.aligner.parameters())
    # state: saved under aligner.*, loaded back
    sd = dp.state_dict()
    assert "aligner.query_layers.4.weight" in sd
    dp2 = vbx.DurationPredictor(num_phoneme_tokens=12, dim_phoneme_emb=64, dim=64, depth=2, dim_head=64, heads=2).cuda()
    dp2.load_state_dict(sd)  # no aligner attached: skipped, as before
    dp2.attach_aligner()
    dp2.load_state_dict(sd)
    assert torch.equal(dp2.aligner.query_layers[4].weight, dp.aligner.query_layers[4].weight)


# ----------------------------------------------------------------------------- learning
def _planted_task(seed=21):
    """mel frames that ARE a fixed projection of the phoneme embedding they sit on, plus noise: a monotonic alignment to find"""
    g = torch.Generator().manual_seed(seed)
    B, T, K, H, C = 2, 67, 17, 64, 80
    keys = torch.randn(B, K, H, generator=g)
    proj = torch.randn(H, C, generator=g) / H ** 0.5
    klens, qlens = [17, 12], [67, 50]
    queries = 0.3 * torch.randn(B, C, T, generator=g)
    for b in range(B):
        t = torch.arange(qlens[b])
        queries[b, :, :qlens[b]] += (keys[b, (t * klens[b]) // qlens[b]] @ proj).t()
    return queries, keys, klens, qlens


def test_twenty_adam_steps_lower_the_forward_sum_loss():
    import align_ref

    queries, keys, klens, qlens = _planted_task()
    sd = R.init_state(80, 64, 80, 31, TAU)
    steps, lr = 20, 1e-3
    # the restatement's own run of the same steps, fp64
    leaves = {n: sd[n].double().requires_grad_() for n in R.PARAMS}
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    mask = R.mask_of(klens, keys.shape[1])
    ref_curve = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = align_ref.forward_sum_ref(R.forward(leaves, queries, keys, mask, TAU)[1][:, 0], klens, qlens)
        ref_curve.append(float(loss.detach()))
        loss.backward()
        opt.step()
    # the device
    mod = _module((80, 64, 80), sd)
    opt = torch.optim.Adam(list(mod.parameters()), lr=lr)
    q, k, m = queries.cuda(), keys.cuda(), mask.cuda()
    kl, ql = torch.tensor(klens, device="cuda"), torch.tensor(qlens, device="cuda")
    fsl, curve = vbx.ForwardSumLoss(), []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = fsl(mod(q, k, m)[1], kl, ql)
        curve.append(loss.detach())
        loss.backward()
        opt.step()
    curve = [float(x) for x in curve]
    print("learning, fp64 restatement:", " ".join(f"{x:.4f}" for x in ref_curve))
    print("learning, device:          ", " ".join(f"{x:.4f}" for x in curve))
    RECORD["learning: forward-sum loss before / after 20 Adam steps, fp64 restatement"] = (ref_curve[0], ref_curve[-1])
    RECORD["learning: forward-sum loss before / after 20 Adam steps, device"] = (curve[0], curve[-1])
    ref_drop, drop = ref_curve[0] - ref_curve[-1], curve[0] - curve[-1]
    assert ref_drop > 0
    # the margin is the restatement's own: a wrong sign does not descend and a lost factor descends about half as far, so at
    # least three quarters of the fp64 run's drop; the two runs differ by operand rounding only
    assert drop >= 0.75 * ref_drop, (drop, ref_drop)
    assert abs(curve[0] - ref_curve[0]) <= R.tolerance() * abs(ref_curve[0])


def test_zz_print_the_record():
    """not a check: the largest measured ratio to every bound and the module's errors (profiles/aligner_parity.txt)"""
    print("\naligner parity, MI355X: the largest value over tests/test_aligner_gpu.py's cases; tolerance "
          f"{R.tolerance():.4f} (a tenth of the smallest planted movement)")
    for key in sorted(RECORD):
        v = RECORD[key]
        print(f"  {key}: " + (f"{v[0]:.4f} -> {v[1]:.4f}" if isinstance(v, tuple) else f"{v:.4g}"))
