"""DurationPredictor training on the device (voicebox_pytorch_amd/duration.py, csrc/duration.hip) against
tests/duration_train_ref.py in fp64: the three kernels per element against the bounds of include/vbx.h, the module's loss and every
parameter gradient through the one compare() that tests/test_duration_train_cpu.py holds against the planted faults, the aligner
branch teacher-forced with the device's own durations, and a short training run.

Measured on an MI355X (profiles/duration_train_parity.txt): the loss within 1.4e-4, every gradient within 0.10 (bound 0.15), to_pred's
within 1.9e-3, the aligner's within 3.5e-3.  These hold with vbx_attn_delta_consistent in the stand-alone stack's backward (include/vbx.h);
with delta taken from the forward's fp16 output the same cases measured up to 0.64.

`pytest -s -m gpu tests/test_duration_train_gpu.py` prints the lines kept in profiles/duration_train_parity.txt (and writes them to
the file named by VBX_DURATION_PARITY_OUT, when set)."""
import os

import pytest
import torch

import align_ref
import aligner_ref
import duration_train_ref as R
from oracle import restate

import voicebox_pytorch_amd as vbx
from voicebox_pytorch_amd import _lib as L
from voicebox_pytorch_amd.masks import rng_override

pytestmark = pytest.mark.gpu

dev = "cuda"
RECORD = {}
LINES = []


def _note(key, value):
    RECORD[key] = max(RECORD.get(key, 0.0), float(value))


def st():
    return L.current_stream()


def _ratio(err, bound):
    return float((err / bound.clamp(min=1e-300)).max())


# ----------------------------------------------------------------------------- the kernels
def _head_fwd(hid, w, b, t, m):
    B, n, D = hid.shape
    d = torch.full((B, n), float("nan"), device=dev)
    num, den, loss = torch.full((B,), float("nan"), device=dev), torch.full((B,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    L.call("vbx_duration_head_fwd", hid, w, b, t, m, d, num, den, loss, B, n, D, st())
    return d, num, den, loss


def _head_bwd(hid, w, d, t, m, den, gscale):
    B, n, D = hid.shape
    dhid = torch.full_like(hid, float("nan"))
    dw, db = torch.full((D,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    scratch = torch.full((L.lib().vbx_duration_head_bwd_scratch_floats(B, n, D),), float("nan"), device=dev)
    L.call("vbx_duration_head_bwd", hid, w, d, t, m, den, gscale, dhid, dw, db, scratch, B, n, D, st())
    return dhid, dw, db


@pytest.mark.parametrize("D", [64, 192, 2048])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 17), (3, 65)])
def test_head_kernels_meet_their_bounds(D, B, n):
    g = torch.Generator().manual_seed(D + 7 * n)
    hid, w, b = torch.randn(B, n, D, generator=g), torch.randn(D, generator=g) * D ** -0.5, torch.randn(1, generator=g)
    t = torch.round(3 * torch.randn(B, n, generator=g))
    m = (torch.rand(B, n, generator=g) < 0.7).to(torch.uint8)
    m[0, 0] = 1
    if B > 1:
        m[B - 1] = 0  # den = 0
    hd, wd, bd, md = hid.to(dev), w.to(dev), b.to(dev), m.to(dev)
    d0 = _head_fwd(hd, wd, bd, t.to(dev), md)[0]
    rd = torch.empty(B, n, device=dev)
    L.call("vbx_rowdot", hd, wd, bd, rd, B * n, D, st())
    assert torch.equal(d0, rd)  # vbx_rowdot's arithmetic: the bits eval mode returns
    t[0, 0] = float(d0[0, 0])  # a position with d == t exactly: sign 0
    td = t.to(dev)
    d, num, den, loss = _head_fwd(hd, wd, bd, td, md)
    assert torch.equal(d, d0)
    d64 = hid.double() @ w.double() + b.double()
    err, bound = (d.cpu().double() - d64).abs(), R.rowdot_bound(hid, w, b)
    assert bool((err <= bound).all()), _ratio(err, bound)
    _note("head forward: |d - fp64| / ((D + 2) u (sum |x w| + |b|))", _ratio(err, bound))
    l64, n64, den64 = R.loss64(d.cpu(), t, m)  # teacher-forced on the kernel's own d
    assert torch.equal(den.cpu().double(), den64)
    assert abs(float(loss) - float(l64)) <= R.loss_bound(l64, B, n), (float(loss), float(l64))
    assert bool(((num.cpu().double() - n64).abs() <= (n + 2) * R.U24 * n64).all())
    _note("head forward: |loss - fp64 on own d| / ((n + B + 4) u loss)", abs(float(loss) - float(l64)) / max(R.loss_bound(l64, B, n), 1e-300))
    gscale = torch.tensor([0.75], device=dev)
    dhid, dw, db = _head_bwd(hd, wd, d, td, md, den, gscale)
    g64, dhid64, dw64, db64, dwabs, dbabs = R.head_bwd_ref(hid, w, d.cpu(), t, m, 0.75)
    err = (dhid.cpu().double() - dhid64).abs()
    assert bool((err <= 3 * R.U24 * dhid64.abs()).all()), _ratio(err, 3 * R.U24 * dhid64.abs())
    assert float(dhid[0, 0].abs().max()) == 0.0 and (B == 1 or float(dhid[B - 1].abs().max()) == 0.0)
    _note("head backward: |dhid - fp64| / (3 u |ref|)", _ratio(err, 3 * R.U24 * dhid64.abs()) if float(dhid64.abs().max()) > 0 else 0.0)
    err, bound = (dw.cpu().double() - dw64).abs(), (B * n + 2) * R.U24 * dwabs
    assert bool((err <= bound).all()), _ratio(err, bound)
    _note("head backward: |dw - fp64| / ((B n + 2) u sum |terms|)", _ratio(err, bound) if float(dwabs.max()) > 0 else 0.0)
    assert abs(float(db) - float(db64)) <= (B * n + 2) * R.U24 * float(dbabs)
    # a NULL gscale is 1; reruns give the same bits; a batch row alone gives the bits it gives inside the batch
    dh1 = _head_bwd(hd, wd, d, td, md, den, None)[0]
    one = _head_bwd(hd, wd, d, td, md, den, torch.ones(1, device=dev))[0]
    assert torch.equal(dh1, one)
    again = _head_fwd(hd, wd, bd, td, md) + _head_bwd(hd, wd, d, td, md, den, gscale)
    assert all(torch.equal(a, b_) for a, b_ in zip(again, (d, num, den, loss, dhid, dw, db)))
    for r in range(B):
        d1, n1, e1, l1 = _head_fwd(hd[r:r + 1].contiguous(), wd, bd, td[r:r + 1].contiguous(), md[r:r + 1].contiguous())
        assert torch.equal(d1[0], d[r]) and torch.equal(n1[0], num[r]) and torch.equal(e1[0], den[r])
        assert float(l1) == float(num[r] / den[r].clamp(min=1e-5))
        gs = torch.tensor([0.75 / B], device=dev)  # the 1 / B of the batch mean, a power-of-two-free factor: compare in fp64 instead
        a1 = _head_bwd(hd[r:r + 1].contiguous(), wd, d1, td[r:r + 1].contiguous(), md[r:r + 1].contiguous(), e1, gs)[0]
        assert bool(((a1[0].double() - dhid[r].double()).abs() <= 4 * R.U24 * dhid[r].double().abs()).all())


@pytest.mark.parametrize("E", [24, 32])
def test_phoneme_emb_bwd_is_the_ordered_sum(E):
    V, B, n = 37, 3, 65
    g = torch.Generator().manual_seed(E)
    ids = torch.randint(0, 29, (B, n), generator=g)  # ids 29 .. 36 unused; repeats everywhere
    ids[1, 40:] = -1
    ids[2, 5:] = -1
    ld = E + 64
    ga_full, gb = torch.randn(B * n, ld, generator=g), torch.randn(B * n, E, generator=g)
    idd = ids.to(dev)
    for a, b in ((ga_full, gb), (ga_full, None), (None, gb)):
        gt = torch.full((V, E), float("nan"), device=dev)
        L.call("vbx_phoneme_emb_bwd", idd, None if a is None else a.to(dev), ld, None if b is None else b.to(dev), gt, B * n, V, E, st())
        ref, ab, count = R.table_grad_ref(ids, None if a is None else a[:, :E], b, V)
        err, bound = (gt.cpu().double() - ref).abs(), (count[:, None] + 2) * R.U24 * ab
        assert bool((err <= bound).all()), _ratio(err, bound)
        assert float(gt[29:].abs().max()) == 0.0 and int(count[0]) > int((ids == 0).sum())  # unused rows 0; padding lands on row 0
        _note("table gradient: |g - fp64| / ((count + 2) u sum |terms|)", _ratio(err[:29], bound[:29]))
        gt2 = torch.full((V, E), float("nan"), device=dev)
        L.call("vbx_phoneme_emb_bwd", idd, None if a is None else a.to(dev), ld, None if b is None else b.to(dev), gt2, B * n, V, E, st())
        assert torch.equal(gt, gt2)
    with pytest.raises(L.VbxError):
        L.call("vbx_phoneme_emb_bwd", idd, None, ld, None, gt, B * n, V, E, st())


@pytest.mark.parametrize("E", [24, 32])
def test_training_pack_writes_the_same_fp16_bits(E):
    B, n, S, D, V = 3, 17, 17, 64, 37
    g = torch.Generator().manual_seed(E + 1)
    ids = torch.randint(-1, V, (B, n), generator=g).to(dev)
    table, cond, null = torch.randn(V, E, generator=g).to(dev), torch.randn(B, S, D, generator=g).to(dev), torch.randn(D, generator=g).to(dev)
    cmask = (torch.rand(B, S, generator=g) < 0.5).to(torch.uint8).to(dev)
    drop = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    a = torch.zeros(B * n, E + D, dtype=torch.float16, device=dev)
    L.call("vbx_pack_phoneme_input", ids, table, E, cond, S, cmask, drop, null, a, B, n, D, st())
    b, bb = torch.zeros_like(a), torch.zeros(B * n, E + D, dtype=torch.bfloat16, device=dev)
    emb = torch.zeros(B, n, E, device=dev)
    L.call("vbx_pack_phoneme_input_train", ids, table, E, cond, S, cmask, drop, null, b, bb, emb, B, n, D, st())
    assert torch.equal(a, b)
    assert torch.equal(emb, table[ids.clamp(min=0)])
    full = torch.cat((emb.reshape(B * n, E), torch.where(drop.bool()[:, None, None], null.expand(B, S, D),
                                                        cond * (cmask == 0)[..., None]).reshape(B * n, D)), 1)
    assert torch.equal(bb, full.to(torch.bfloat16)) and torch.equal(a, full.to(torch.float16))
    c = torch.zeros_like(a)
    L.call("vbx_pack_phoneme_input_train", ids, table, E, cond, S, cmask, drop, null, c, None, None, B, n, D, st())
    assert torch.equal(a, c)


@pytest.mark.parametrize("B,H,Np,masked", [(2, 2, 1, False), (1, 2, 65, True), (2, 1, 130, True), (1, 1, 256, False)])
def test_consistent_delta_is_the_sum_over_the_backwards_own_operands(B, H, Np, masked):
    """vbx_attn_delta_consistent against sum_j P dP in fp64 on the same fp16 / bf16 operands and the same fp32 lse.  Per query:
    s and dP are 64-term fp32 fma chains (66 u sum |terms|), s - L one more rounding, exp2 the hardware's (4 u allowed), the sum over
    the keys Np + 4 roundings: |err| <= sum_j p_j ((ln 2 (66 u sum_d |q k| + u (|s| + |L|)) + 4 u) |dP_j| + 66 u sum_d |dO v|)
    + (Np + 4) u sum_j p_j |dP_j|.  At one token delta must equal dO . v to that bound: what makes dS vanish there."""
    g = torch.Generator().manual_seed(Np)
    q = (torch.randn(B, H, Np, 64, generator=g) * 1.5).half()
    k = torch.randn(B, H, Np, 64, generator=g).half()
    v = torch.randn(B, H, Np, 64, generator=g).bfloat16()
    dO = torch.randn(B * Np, H * 64, generator=g).bfloat16()
    mask = torch.ones(B, Np, dtype=torch.bool)
    if masked:
        mask[0, Np // 2:Np // 2 + 7] = False
    s = q.double() @ k.double().transpose(2, 3)  # log2 domain: the fp16 q operand carries its prescale
    sm = s.masked_fill(~mask[:, None, None, :], -float("inf"))
    lse = (torch.logsumexp(sm * 0.6931471805599453, -1) / 0.6931471805599453).float()
    p = torch.exp2(sm - lse.double()[..., None])
    g4 = dO.double().view(B, Np, H, 64).transpose(1, 2)
    dp = g4 @ v.double().transpose(2, 3)
    ref = (p * dp).sum(-1)
    delta = torch.full((B, H, Np), float("nan"), device=dev)
    args = (q.to(dev), k.to(dev), v.to(dev), mask.to(torch.uint8).to(dev) if masked else None, dO.to(dev), lse.to(dev))
    L.call("vbx_attn_delta_consistent", *args, delta, B, H, Np, st())
    u = R.U24
    sabs = q.double().abs() @ k.double().abs().transpose(2, 3)
    dpabs = g4.abs() @ v.double().abs().transpose(2, 3)
    per_key = (0.6931471805599453 * (66 * u * sabs + u * (s.abs() + lse.double().abs()[..., None])) + 4 * u) * dp.abs() + 66 * u * dpabs
    bound = (p * per_key).sum(-1) + (Np + 4) * u * (p * dp.abs()).sum(-1)
    err = (delta.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), _ratio(err, bound)
    _note("consistent delta: |delta - fp64| / bound", _ratio(err, bound))
    again = torch.full((B, H, Np), float("nan"), device=dev)
    L.call("vbx_attn_delta_consistent", *args, again, B, H, Np, st())
    assert torch.equal(delta, again)


# ----------------------------------------------------------------------------- the module, given durations
def _module(state, E, aligner_state=None, **kw):
    dp = vbx.DurationPredictor(num_phoneme_tokens=37, dim_phoneme_emb=E, dim=64, depth=2, dim_head=64, heads=2,
                               aligner_kwargs=dict(R.ALIGNER_DIMS), **kw)
    dp.load_state_dict(state)
    dp = dp.to(dev)
    if aligner_state is not None:
        dp.attach_aligner().load_state_dict(aligner_state)
    return dp.train()


def _grads(dp):
    return {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in dp.named_parameters() if p.requires_grad}


def _log(title, loss, ref, figures):
    new = {k: v for k, v in figures.items() if k.startswith(R.NEW_STAGES)}
    stack = {k: v for k, v in figures.items() if k.startswith("transformer.")}
    al = {k: v for k, v in figures.items() if k.startswith("aligner.")}
    line = (f"{title}: loss {float(loss):.6f} vs {float(ref):.6f} (rel {figures['loss']:.2e}); gradients, relative L2: "
            + ", ".join(f"{k} {v:.3e}" for k, v in sorted(new.items())) + f"; stack worst {max(stack.values()):.3e}"
            + (f"; aligner worst {max(al.values()):.3e}" if al else ""))
    print(line)
    LINES.append(line)
    for k, v in new.items():
        _note(f"given / aligner cases, worst relative L2 of d {k}", v)
    _note("given / aligner cases, worst relative L2 over the stack's tensors", max(stack.values()))
    if figures.get("transformer.layers.0.3.k_norm.gamma") is not None and "1x1" in title:
        _note("1x1 cases, zero-reference q_norm / k_norm gamma: norm / (2^-8 |whole reference gradient|)",
              max(v for k, v in figures.items() if k.endswith(("q_norm.gamma", "k_norm.gamma"))))


@pytest.mark.parametrize("E,B,n,drop", R.GIVEN_CASES, ids=[f"E{E}_{B}x{n}_drop{int(d)}" for E, B, n, d in R.GIVEN_CASES])
def test_given_durations_loss_and_gradients(E, B, n, drop):
    case, ref = R.given_case(E, B, n, drop), R.given_reference(E, B, n, drop)
    assert R.margin(ref["d"], case["target"]) >= 0.5 - 1e-9  # no loss row near a sign change, none left out
    dp = _module(case["state"], E)
    loss = dp(cond=case["cond"].to(dev), phoneme_ids=case["ids"].to(dev), target=case["target"].to(dev),
              cond_mask=case["cond_mask"].to(dev), cond_drop_prob=1.0 if drop else 0.0)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "cuda"
    loss.backward()
    got = dict(loss=loss.detach().cpu(), grads=_grads(dp))
    assert dp.null_cond.grad is None
    for name in ("to_pred.0.weight", "to_pred.0.bias", "conv_embed.dw_conv1d.0.weight", "conv_embed.dw_conv1d.0.bias", "to_embed.weight",
                 "to_embed.bias", "to_phoneme_emb.weight"):
        assert got["grads"][name] is not None, name
    assert all(v is not None for k, v in got["grads"].items() if k.startswith("transformer."))
    problems, figures = R.compare(got, ref)
    _log(f"given durations E={E} {B}x{n} cond_drop_prob={int(drop)}", loss, ref["loss"], figures)
    assert problems == [], problems
    used = torch.zeros(37, dtype=torch.bool)
    used[case["ids"].clamp(min=0).reshape(-1)] = True
    assert float(got["grads"]["to_phoneme_emb.weight"][~used].abs().max()) == 0.0  # rows of unused ids: exactly 0


def test_given_durations_integer_targets_and_drawn_masks():
    """an int64 target gives the bits of the float one; the random cond_mask branch keeps its take_draw hooks: injected draws equal
    the explicit mask bit for bit; an eval forward in between leaves training untouched"""
    E, B, n = 32, 3, 17
    case = R.given_case(E, B, n, False)
    dp = _module(case["state"], E)
    cond, ids, t = case["cond"].to(dev), case["ids"].to(dev), case["target"].to(dev)
    a = dp(cond=cond, phoneme_ids=ids, target=t, cond_mask=case["cond_mask"].to(dev))
    b = dp(cond=cond, phoneme_ids=ids, target=t.long(), cond_mask=case["cond_mask"].to(dev))
    assert torch.equal(a, b)
    frac, rand = torch.tensor([0.3, 0.6, 0.9]), torch.tensor([0.1, 0.5, 0.8])
    with rng_override(coin=True, frac_lengths=frac, rand=rand):
        c = dp(cond=cond, phoneme_ids=ids, target=t)
    em = restate.frac_lengths_mask(n, frac, rand).to(dev)
    assert torch.equal(c, dp(cond=cond, phoneme_ids=ids, target=t, cond_mask=em))
    with rng_override(cond_drop=torch.tensor([True, False, True])):
        e = dp(cond=cond, phoneme_ids=ids, target=t, cond_mask=em, cond_drop_prob=0.5)
    assert bool(torch.isfinite(e)) and not torch.equal(e, c)


@pytest.mark.parametrize("E,B,n,drop", [(24, 3, 17, False), (32, 2, 65, True), (32, 1, 1, False)])
def test_front_end_node_alone(E, B, n, drop):
    """pack -> to_embed -> conv_embed + residual as its own autograd node, given upstream gradients for both outputs: the forward
    within fp32 accumulation of the restatement on the same fp16 operands (K = E + D <= 96 products: 1e-5), the fp32 gradients
    (conv, to_embed.bias) within 1e-5, and the two bf16 GEMMs per element within BF16_PRODUCT sum |terms| -- the to_embed weight
    gradient, and the table gradient that adds the dgrad's columns 0:E to the second consumer's gradient"""
    from voicebox_pytorch_amd.duration import _FrontEndFn

    case = R.given_case(E, B, n, drop)
    dp = _module(case["state"], E)
    cond, ids, _, cmask, dr, _, am8 = dp._resolve(case["cond"], case["ids"], case["cond_mask"], 1.0 if drop else 0.0, None)
    conv = dp.conv_embed.dw_conv1d[0]
    x, emb = _FrontEndFn.apply(dp, ids, cond, cmask, dr, am8, True, dp.to_phoneme_emb.weight, dp.to_embed.weight, dp.to_embed.bias,
                               conv.weight, conv.bias)
    g = torch.Generator().manual_seed(n)
    gx, ge = torch.randn(B, n, 64, generator=g), torch.randn(B, n, E, generator=g)
    torch.autograd.backward([x, emb], [gx.to(dev), ge.to(dev)])
    p = R.leaves(case["state"])
    with restate.emulate_fp16_operands():
        x64, e64, emb64, packed = R.front_end(p, case)
    live = (case["ids"] != -1)[..., None]
    assert R.rel_l2(x.detach().cpu() * live, x64.detach() * live) < 1e-5
    assert torch.equal(emb.detach().cpu().double(), emb64.detach())
    de = torch.autograd.grad(x64, e64, gx.double(), retain_graph=True)[0]
    torch.autograd.backward([x64, emb64], [gx.double(), ge.double()])
    got = _grads(dp)
    for k in ("conv_embed.dw_conv1d.0.weight", "conv_embed.dw_conv1d.0.bias", "to_embed.bias"):
        assert R.rel_l2(got[k], p[k].grad) < 1e-5, (k, R.rel_l2(got[k], p[k].grad))
        _note(f"front end alone: relative L2 of d {k}", R.rel_l2(got[k], p[k].grad))
    de2, pk2 = de.reshape(B * n, 64), packed.detach().reshape(B * n, E + 64)
    err, bound = (got["to_embed.weight"].double() - p["to_embed.weight"].grad).abs(), R.BF16_PRODUCT * (de2.abs().t() @ pk2.abs())
    assert bool((err <= bound).all()), _ratio(err, bound)
    _note("front end alone: |d to_embed.weight - fp64| / (BF16_PRODUCT sum |terms|)", _ratio(err, bound))
    w = p["to_embed.weight"].detach()[:, :E]
    row_bound = R.BF16_PRODUCT * (de2.abs() @ w.abs())  # of every row of the dgrad
    _, ab, count = R.table_grad_ref(case["ids"], (de2 @ w), ge.reshape(B * n, E), 37)
    tb = torch.zeros(37, E, dtype=torch.float64).index_add_(0, case["ids"].clamp(min=0).reshape(-1), row_bound) + (count[:, None] + 2) * R.U24 * ab
    err = (got["to_phoneme_emb.weight"].double() - p["to_phoneme_emb.weight"].grad).abs()
    assert bool((err <= tb).all()), _ratio(err, tb)
    _note("front end alone: |d to_phoneme_emb.weight - fp64| / bound", _ratio(err, tb))
    _note("front end alone: relative L2 of d to_embed.weight", R.rel_l2(got["to_embed.weight"], p["to_embed.weight"].grad))
    _note("front end alone: relative L2 of d to_phoneme_emb.weight", R.rel_l2(got["to_phoneme_emb.weight"], p["to_phoneme_emb.weight"].grad))


# ----------------------------------------------------------------------------- the module, aligner branch
@pytest.mark.parametrize("flag", [False, True], ids=["l1_only", "with_align_loss"])
def test_aligner_branch(flag):
    E = 24
    case = R.aligner_case(E, flag=flag)
    al = case["aligner"]
    B, n = case["ids"].shape
    T = al["mel"].shape[1]
    dp = _module(case["state"], E, aligner_state=al["state"])
    ids, mel = case["ids"].to(dev), al["mel"].to(dev)
    pmask = aligner_ref.mask_of(al["klens"], n)[:, None].to(torch.int32).to(dev)
    mmask = aligner_ref.mask_of(al["qlens"], T)[:, None].to(torch.int32).to(dev)
    plen, mlen = torch.tensor(al["klens"], device=dev), torch.tensor(al["qlens"], device=dev)
    # the device's path is bit-equal to the fp64 search on the device's own soft map; the reference is teacher-forced with it
    with torch.no_grad():
        hard, soft, _, _ = dp.forward_aligner(dp.to_phoneme_emb.weight[ids.clamp(min=0)], pmask, mel, mmask)
    want = align_ref.maximum_path_batch_ref(soft.transpose(1, 2).cpu().double(), al["qlens"], al["klens"])[1]
    assert torch.equal(hard.cpu(), want.float())
    tf = dict(case, aligner=dict(al, durations=hard.cpu()))
    ref = R.reference(tf)
    assert float((ref["d"] - 2.5).abs().max()) <= 0.1 and float((ref["d"] - ref["target"]).abs().min()) >= 0.4
    loss = dp(cond=case["cond"].to(dev), phoneme_ids=ids, cond_mask=case["cond_mask"].to(dev), mel=mel, phoneme_len=plen, mel_len=mlen,
              phoneme_mask=pmask, mel_mask=mmask, target=torch.full((B, n), 1e9, device=dev),  # ignored, as in the reference
              return_aligned_phoneme_ids=flag)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    got = dict(loss=loss.detach().cpu(), grads=_grads(dp))
    problems, figures = R.compare(got, ref, aligner_tol=aligner_ref.tolerance())
    _log(f"aligner branch E={E} {B}x{n} T={T} return_aligned_phoneme_ids={flag}", loss, ref["loss"], figures)
    assert problems == [], problems
    if not flag:
        assert all(p.grad is None for p in dp.aligner.parameters())
    else:
        assert all(p.grad is not None for p in dp.aligner.parameters())
        # the table gradient holds both consumers: the L1 part alone is a different tensor, and the reference without the aligner's
        # share is far outside the tolerance
        one = R.reference(tf, fault="emb_one_consumer")["grads"]["to_phoneme_emb.weight"]
        assert R.rel_l2(got["grads"]["to_phoneme_emb.weight"], one) > R.GRAD_TOL
        l1 = R.reference(dict(tf, aligner=dict(tf["aligner"], flag=False)))
        assert abs(float(loss) - float(l1["loss"]) - float(ref["align"])) <= R.LOSS_TOL * float(ref["loss"])


# ----------------------------------------------------------------------------- a training run
def _train(case, seed, steps=R.TRAIN_STEPS, **kw):
    torch.manual_seed(seed)
    dp = _module(case["state"], 32, **kw)
    opt = torch.optim.Adam([p for p in dp.parameters() if p.requires_grad], lr=R.TRAIN_LR)
    args = dict(cond=case["cond"].to(dev), phoneme_ids=case["ids"].to(dev), target=case["target"].to(dev), cond_mask=case["cond_mask"].to(dev))
    losses = []
    for step in range(steps + 1):
        loss = dp(**args)
        losses.append(loss.detach())
        if step < steps:
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
    return torch.stack(losses).cpu()


def test_training_run_learns_and_repeats():
    case = R.train_case()
    ref = R.train_run_ref(case)
    a, b = _train(case, 0), _train(case, 0)
    line = (f"training run 3x17, Adam lr {R.TRAIN_LR}, {R.TRAIN_STEPS} steps: fp64 {ref[0]:.4f} -> {ref[-1]:.4f} ({ref[-1] / ref[0]:.3f} x), "
            f"device {float(a[0]):.4f} -> {float(a[-1]):.4f} ({float(a[-1] / a[0]):.3f} x)")
    print(line)
    print("  fp64  ", [round(x, 4) for x in ref])
    print("  device", [round(float(x), 4) for x in a])
    LINES.append(line)
    assert ref[-1] <= 0.25 * ref[0]
    assert float(a[-1]) <= 0.5 * float(a[0])
    assert torch.equal(a, b)  # the same seed: the same bits
    c, d = _train(case, 1, steps=3, ff_dropout=0.1), _train(case, 1, steps=3, ff_dropout=0.1)
    assert torch.equal(c, d) and not torch.equal(c[:4], a[:4])  # dropout is live in train(), and seeded


def test_zz_report():
    """not a check: the measured values (profiles/duration_train_parity.txt)"""
    out = ["DurationPredictor training parity, MI355X: tests/test_duration_train_gpu.py against tests/duration_train_ref.py (fp64, GEMM "
           f"operand roundings emulated); bounds: loss {R.LOSS_TOL} relative, gradients {R.GRAD_TOL} relative L2 per tensor, aligner.* "
           f"{aligner_ref.tolerance():.4f}"] + LINES
    out += [f"largest over all cases -- {k}: {RECORD[k]:.4g}" for k in sorted(RECORD)]
    print("\n" + "\n".join(out))
    path = os.environ.get("VBX_DURATION_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(out) + "\n")
