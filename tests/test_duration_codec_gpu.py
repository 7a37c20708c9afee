"""DurationPredictor over codec latents on the device (DurationPredictor.attach_codec, csrc/duration.hip:
vbx_pack_phoneme_latent[_train]) against tests/duration_codec_ref.py in fp64 and the fixture of the unmodified reference
(tests/golden/duration_codec.pt): the pack kernel per element against the bound of include/vbx.h, eval against the reference, the
front-end autograd node alone with the derived bound on d proj_in.weight / bias, the module's loss and every gradient in both
training branches, latent_dim == dim bit for bit, and wave -> phonemes -> sample end to end.

`pytest -s -m gpu tests/test_duration_codec_gpu.py` prints the lines kept in profiles/duration_codec_parity.txt (and writes them to
the file named by VBX_DURATION_CODEC_PARITY_OUT, when set).

Measured on an MI355X (profiles/duration_codec_parity.txt): the projected columns reach 0.95 of their bound (the store's rounding),
d proj_in.weight / bias of the node alone 0.073 of theirs (relative L2 3.4e-3 / 2.6e-3); through the module the loss is within 6.4e-5,
proj_in.* within 9.7e-3 and every other gradient within 2.6e-2 (bound 0.15); the reference's d1 / d_null / d3 within 8.3e-3 / 8.3e-3 /
1.3e-2 (bounds 2e-2 / 2e-2 / 4e-2), d1 within 6.2e-4 of the emulated-operand restatement (bound 5e-3)."""
import os

import pytest
import torch

import align_ref
import aligner_ref
import duration_codec_ref as C
import duration_train_ref as R
from oracle import restate
from toy_codec import ToyCodec

import voicebox_pytorch_amd as vbx
from voicebox_pytorch_amd import _lib as L_
from voicebox_pytorch_amd.masks import rng_override

pytestmark = pytest.mark.gpu

dev = "cuda"
RECORD = {}
LINES = []
D = 64
KW = dict(num_phoneme_tokens=37, dim_phoneme_emb=32, dim=64, depth=2, dim_head=64, heads=2)


def _note(key, value):
    RECORD[key] = max(RECORD.get(key, 0.0), float(value))


def st():
    return L_.current_stream()


def _ratio(err, bound):
    return float((err / bound.clamp(min=1e-300)).max())


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


# ----------------------------------------------------------------------------- 1: the pack kernel alone
def _pack_weight(w):
    Dw, L = w.shape
    Kp = L_.lib().vbx_proj_in_kp(L)
    pack = torch.full((Dw, Kp), float("nan"), dtype=torch.float16, device=dev)
    L_.call("vbx_pack_weight", w.to(dev).contiguous(), Dw, L, None, pack, Dw, Kp, 0, 0, st())
    return pack


def _pack_eval(a, rows=slice(None)):
    ids, lat, cm = a["ids"][rows].contiguous(), a["lat"][rows].contiguous(), a["cmask"][rows].contiguous()
    drop = None if a["drop"] is None else a["drop"][rows].contiguous()
    B, n = ids.shape
    out = torch.full((B * n, a["E"] + D), float("nan"), dtype=torch.float16, device=dev)
    L_.call("vbx_pack_phoneme_latent", ids, a["table"], a["E"], lat, lat.shape[1], lat.shape[2], a["w16"], a["bias"], cm, drop, a["null"], out,
            B, n, D, st())
    return out


def _pack_train(a, want_emb=True):
    B, n = a["ids"].shape
    E, Kp = a["E"], a["w16"].shape[1]
    out = torch.full((B * n, E + D), float("nan"), dtype=torch.float16, device=dev)
    outb = torch.full((B * n, E + D), float("nan"), dtype=torch.bfloat16, device=dev)
    emb = torch.full((B, n, E), float("nan"), device=dev) if want_emb else None
    lcb = torch.full((B * n, Kp), float("nan"), dtype=torch.bfloat16, device=dev)
    L_.call("vbx_pack_phoneme_latent_train", a["ids"], a["table"], E, a["lat"], a["lat"].shape[1], a["lat"].shape[2], a["w16"], a["bias"],
            a["cmask"], a["drop"], a["null"], out, outb, emb, lcb, B, n, D, st())
    return out, outb, emb, lcb


PACK_CASES = [(100, 32, 1, 1, 1), (8, 24, 3, 17, 17), (128, 32, 2, 65, 65), (100, 32, 2, 21, 13), (100, 32, 2, 21, 40), (1024, 32, 1, 33, 33)]


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("L,E,B,n,S", PACK_CASES, ids=[f"L{c[0]}_E{c[1]}_{c[2]}x{c[3]}_S{c[4]}" for c in PACK_CASES])
def test_pack_kernel_alone(L, E, B, n, S, drop):
    V = 37
    g = torch.Generator().manual_seed(L + 3 * n + S)
    ids = torch.randint(-1, V, (B, n), generator=g)
    table, lat = torch.randn(V, E, generator=g), torch.randn(B, S, L, generator=g)
    w, bias, null = torch.randn(D, L, generator=g) * L ** -0.5, torch.randn(D, generator=g) * 0.5, torch.randn(D, generator=g)
    cmask = torch.rand(B, S, generator=g) < 0.5
    cmask[0, 0] = S > 2  # a masked row where there is room for one, and a row that counts in every case
    if S > 2:
        cmask[0, 1] = False
    dmask = torch.tensor([b % 2 == 0 for b in range(B)]) if drop else None  # with B > 1 a dropped and a kept sample side by side
    a = dict(E=E, ids=ids.to(dev), table=table.to(dev), lat=lat.to(dev), w16=_pack_weight(w), bias=bias.to(dev), null=null.to(dev),
             cmask=cmask.to(torch.uint8).to(dev), drop=None if dmask is None else dmask.to(torch.uint8).to(dev))
    Kp = a["w16"].shape[1]
    assert Kp % 32 == 0 and Kp > L and torch.equal(a["w16"][:, :L].cpu(), w.half()) and not a["w16"][:, L:].any()
    out = _pack_eval(a)
    # columns 0:E: the bits of vbx_pack_phoneme_input
    old = torch.full((B * n, E + D), float("nan"), dtype=torch.float16, device=dev)
    L_.call("vbx_pack_phoneme_input", a["ids"], a["table"], E, torch.zeros(B, S, D, device=dev), S, a["cmask"], a["drop"], a["null"], old, B, n, D, st())
    assert torch.equal(out[:, :E], old[:, :E]) and torch.equal(out[:, :E].cpu(), table[ids.clamp(min=0)].reshape(B * n, E).half())
    # columns E: per element against fp64 on the same fp16-rounded operands
    lat16, w16 = lat.half().double(), w.half().double()
    y = lat16 @ w16.t() + bias.double()
    bound = restate.curtail_or_pad(C.proj_bound(lat16, w16, bias.double(), y), n)
    y = restate.curtail_or_pad(y, n)
    got = out[:, E:].reshape(B, n, D).cpu()
    pos = torch.arange(n)[None, :].expand(B, n)
    padded = pos >= S
    dropped = (dmask[:, None].expand(B, n) if drop else torch.zeros(B, n, dtype=torch.bool)) & ~padded
    masked = restate.curtail_or_pad(cmask[..., None].double(), n)[..., 0].bool() & ~padded & ~dropped
    live = ~(padded | dropped | masked)
    assert not got[padded].any() and not got[masked].any()  # exactly 0: not the bias, and not null_cond past S
    assert torch.equal(got[dropped], null.half().expand(B, n, D)[dropped])
    assert int(live.sum()) > 0 or (drop and B == 1)
    err = (got.double() - y).abs()
    assert bool((err[live] <= bound[live]).all()), _ratio(err[live], bound[live])
    if int(live.sum()):
        _note("pack: |cond'' - fp64| / ((L + 2) u (sum |w x| + |b|) + 2^-11 |y|)", _ratio(err[live], bound[live]))
        assert float(got[live].abs().max()) > 0
    # the training variant: the same fp16 bits, the bf16 copy, the embedding rows, the weight-gradient operand
    out_t, outb, emb, lcb = _pack_train(a)
    assert torch.equal(out_t, out)
    assert torch.equal(emb.cpu(), table[ids.clamp(min=0)])
    assert torch.equal(outb[:, :E].cpu(), table[ids.clamp(min=0)].reshape(B * n, E).bfloat16())
    gb = outb[:, E:].reshape(B, n, D).cpu()
    assert not gb[padded].any() and not gb[masked].any() and torch.equal(gb[dropped], null.bfloat16().expand(B, n, D)[dropped])
    # one rounding of the same fp32 value to bf16's 8 significant bits (unit roundoff 2^-8) instead of fp16's 11 (2^-11)
    errb, boundb = (gb.double() - y).abs(), bound + (R.U_BF16 - 2.0 ** -11) * y.abs()
    assert bool((errb[live] <= boundb[live]).all()), _ratio(errb[live], boundb[live])
    want = torch.zeros(B * n, Kp, dtype=torch.bfloat16)
    want[:, :L + 1] = C.lcb_rows(lat, cmask, dmask, n).float().bfloat16()
    assert torch.equal(lcb.cpu(), want)
    assert int((lcb[:, L] == 1).sum()) == int(live.sum())  # column L: one per row that counts
    out_n = _pack_train(a, want_emb=False)
    assert torch.equal(out_n[0], out) and torch.equal(out_n[1], outb) and torch.equal(out_n[3], lcb)
    # reruns, and a batch row alone
    assert torch.equal(_pack_eval(a), out)
    for b in range(B):
        assert torch.equal(_pack_eval(a, slice(b, b + 1)), out[b * n:(b + 1) * n])


def test_pack_kernel_refuses_what_it_does_not_serve():
    a = dict(ids=torch.zeros(1, 2, dtype=torch.long, device=dev), table=torch.zeros(37, 32, device=dev), bias=torch.zeros(64, device=dev),
             null=torch.zeros(64, device=dev), out=torch.zeros(2, 96, dtype=torch.float16, device=dev))
    for L, Dd, E in ((4, 64, 32), (1025, 64, 32), (100, 96, 32), (100, 64, 12)):
        lat, w16 = torch.zeros(1, 2, L, device=dev), torch.zeros(128, 1088, dtype=torch.float16, device=dev)
        with pytest.raises(L_.VbxError):
            L_.call("vbx_pack_phoneme_latent", a["ids"], a["table"], E, lat, 2, L, w16, a["bias"], None, None, a["null"], a["out"], 1, 2, Dd, st())


# ----------------------------------------------------------------------------- 2: eval against the reference fixture
def _fixture_module(c):
    dp = vbx.DurationPredictor(**KW).attach_codec(ToyCodec(c["latent_dim"]))
    missing = dp.load_state_dict(c["state"], strict=False)
    assert not missing.unexpected_keys and all("inv_freq" in k for k in missing.missing_keys), missing
    return dp.to(dev).eval()


def test_eval_against_the_reference_fixture(golden):
    for name, c in C.fixture_cases(golden("duration_codec")).items():
        dp = _fixture_module(c)
        ids, cond, cm = c["ids"].to(dev), c["cond"].to(dev), c["cond_mask"].to(dev)
        d1 = dp(cond=cond, phoneme_ids=ids, cond_mask=cm)
        dn = dp(cond=cond, phoneme_ids=ids, cond_mask=cm, cond_drop_prob=1.0)
        d3, aligned = dp.forward_with_cond_scale(cond=cond, phoneme_ids=ids, cond_mask=cm, cond_scale=3.0, return_aligned_phoneme_ids=True)
        assert d1.shape == c["d1"].shape and d1.dtype == torch.float32
        e1, en, e3 = rel(d1, c["d1"]), rel(dn, c["d_null"]), rel(d3, c["d3"])
        line = f"eval {name}: relative L2 to the reference d1 {e1:.3e}, d_null {en:.3e}, d3 {e3:.3e}"
        with torch.no_grad(), restate.emulate_fp16_operands():
            de = C.predict({k: v.double() if v.is_floating_point() else v for k, v in c["state"].items()}, R.cfg_of(), c)
        ee = rel(d1, de)
        line += f"; d1 to the emulated-operand restatement {ee:.3e}"
        print(line)
        LINES.append(line)
        assert e1 < 2e-2 and en < 2e-2 and e3 < 4e-2, (name, e1, en, e3)
        assert ee < R.LOSS_TOL, (name, ee)
        assert torch.equal(dp.align_phoneme_ids_with_durations(ids, c["d3"].to(dev)).cpu(), c["aligned"]), name
        assert torch.equal(aligned.cpu(), restate.align_phoneme_ids_with_durations(c["ids"], d3.cpu())), name
        frac, rand = torch.tensor([0.3, 0.6, 0.9]), torch.tensor([0.1, 0.5, 0.8])
        with rng_override(coin=True, frac_lengths=frac, rand=rand):
            dr = dp(cond=cond, phoneme_ids=ids)
        em = restate.frac_lengths_mask(cond.shape[1], frac, rand).to(dev)
        assert torch.equal(dr, dp(cond=cond, phoneme_ids=ids, cond_mask=em)), name
        with pytest.raises(AssertionError, match="latent_dim"):
            dp(cond=torch.zeros(3, 5, 64, device=dev), phoneme_ids=ids, cond_mask=torch.zeros(3, 5, dtype=torch.bool, device=dev))
        # the fp16 pack of proj_in.weight follows the parameter: an in-place update and load_state_dict both invalidate it
        with torch.no_grad():
            dp.proj_in.weight.mul_(0.5)
        moved = dp(cond=cond, phoneme_ids=ids, cond_mask=cm)
        fresh = _fixture_module(dict(c, state={**c["state"], "proj_in.weight": c["state"]["proj_in.weight"] * 0.5}))
        assert not torch.equal(moved, d1) and torch.equal(moved, fresh(cond=cond, phoneme_ids=ids, cond_mask=cm))
        dp.load_state_dict(c["state"], strict=False)
        assert torch.equal(dp(cond=cond, phoneme_ids=ids, cond_mask=cm), d1)


# ----------------------------------------------------------------------------- 3: the front-end node alone
def _module(state, E, L=None, aligner_state=None, **kw):
    dp = vbx.DurationPredictor(num_phoneme_tokens=37, dim_phoneme_emb=E, dim=64, depth=2, dim_head=64, heads=2,
                               aligner_kwargs=dict(R.ALIGNER_DIMS), **kw)
    if L is not None:
        dp.attach_codec(ToyCodec(L))
    dp.load_state_dict(state)
    dp = dp.to(dev)
    if aligner_state is not None:
        dp.attach_aligner().load_state_dict(aligner_state)
    return dp.train()


def _grads(dp):
    return {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in dp.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("L,E,B,n,drop", [(100, 24, 3, 17, False), (128, 32, 2, 65, True), (8, 32, 1, 1, False)])
def test_front_end_node_alone(L, E, B, n, drop):
    """tests/test_duration_train_gpu.py::test_front_end_node_alone with proj_in in front, its bounds unchanged: the forward within
    fp32 accumulation of the restatement ON THE SAME fp16 OPERANDS (1e-5) -- the restatement's to_embed reads the cond'' columns the
    pack kernel wrote (test_pack_kernel_alone holds them to their own bound; recomputed in fp64 an element may round to the
    neighbouring fp16 value) -- the fp32 gradients within 1e-5, the bf16 GEMMs per element within BF16_PRODUCT sum |terms|.  New:
    d proj_in.weight / bias per element to duration_codec_ref.proj_wgrad_bound, exactly 0 when every sample is dropped."""
    from voicebox_pytorch_amd.duration import _FrontEndFn

    case = C.given_case(L, E, B, n, drop)
    dp = _module(case["state"], E, L)
    cond, ids, _, cmask, dr, _, am8 = dp._resolve(case["cond"], case["ids"], case["cond_mask"], 1.0 if drop else 0.0, None)
    conv = dp.conv_embed.dw_conv1d[0]
    x, emb = _FrontEndFn.apply(dp, ids, cond, cmask, dr, am8, True, dp.to_phoneme_emb.weight, dp.to_embed.weight, dp.to_embed.bias,
                               conv.weight, conv.bias, dp.proj_in.weight, dp.proj_in.bias)
    g = torch.Generator().manual_seed(n)
    gx, ge = torch.randn(B, n, 64, generator=g), torch.randn(B, n, E, generator=g)
    torch.autograd.backward([x, emb], [gx.to(dev), ge.to(dev)])
    p = R.leaves(case["state"])
    pw16, pb32 = dp._proj_operands()
    dev16 = torch.empty(B * n, E + 64, dtype=torch.float16, device=dev)
    L_.call("vbx_pack_phoneme_latent", ids, dp.to_phoneme_emb.weight.detach(), E, cond, n, L, pw16, pb32, cmask, dr, dp.null_cond.detach(),
            dev16, B, n, 64, st())
    with restate.emulate_fp16_operands():
        x64, e64, emb64, packed, c64 = C.front_end(p, case, cond16=dev16[:, E:].reshape(B, n, 64).cpu())
    live = (case["ids"] != -1)[..., None]
    fwd = R.rel_l2(x.detach().cpu() * live, x64.detach() * live)
    assert fwd < 1e-5, fwd
    _note("front end alone: relative L2 of x (bound 1e-5)", fwd)
    assert torch.equal(emb.detach().cpu().double(), emb64.detach())
    de, dc = torch.autograd.grad(x64, (e64, c64), gx.double(), retain_graph=True)
    torch.autograd.backward([x64, emb64], [gx.double(), ge.double()])
    got = _grads(dp)
    assert dp.null_cond.grad is None
    for k in ("conv_embed.dw_conv1d.0.weight", "conv_embed.dw_conv1d.0.bias", "to_embed.bias"):
        assert R.rel_l2(got[k], p[k].grad) < 1e-5, (k, R.rel_l2(got[k], p[k].grad))
    de2, dc2, pk2 = de.reshape(B * n, 64), dc.reshape(B * n, 64), packed.detach().reshape(B * n, E + 64)
    err, bound = (got["to_embed.weight"].double() - p["to_embed.weight"].grad).abs(), R.BF16_PRODUCT * (de2.abs().t() @ pk2.abs())
    assert bool((err <= bound).all()), _ratio(err, bound)
    _note("front end alone: |d to_embed.weight - fp64| / bound", _ratio(err, bound))
    w = p["to_embed.weight"].detach()[:, :E]
    row_bound = R.BF16_PRODUCT * (de2.abs() @ w.abs())
    _, ab, count = R.table_grad_ref(case["ids"], (de2 @ w), ge.reshape(B * n, E), 37)
    tb = torch.zeros(37, E, dtype=torch.float64).index_add_(0, case["ids"].clamp(min=0).reshape(-1), row_bound) + (count[:, None] + 2) * R.U24 * ab
    err = (got["to_phoneme_emb.weight"].double() - p["to_phoneme_emb.weight"].grad).abs()
    assert bool((err <= tb).all()), _ratio(err, tb)
    _note("front end alone: |d to_phoneme_emb.weight - fp64| / bound", _ratio(err, tb))
    # proj_in
    xr = C.lcb_rows(case["cond"], case["cond_mask"], case.get("drop"), n).float().bfloat16().double()
    bound = C.proj_wgrad_bound(de2, p["to_embed.weight"].detach()[:, E:], dc2, xr)
    got_p = torch.cat((got["proj_in.weight"].double(), got["proj_in.bias"].double()[:, None]), dim=1)
    ref_w = p["proj_in.weight"].grad if p["proj_in.weight"].grad is not None else torch.zeros(64, L, dtype=torch.float64)
    ref_b = p["proj_in.bias"].grad if p["proj_in.bias"].grad is not None else torch.zeros(64, dtype=torch.float64)
    ref_p = torch.cat((ref_w, ref_b[:, None]), dim=1)
    err = (got_p - ref_p).abs()
    assert bool((err <= bound).all()), _ratio(err, bound)
    if not xr.any():  # every sample dropped, or the single row of the 1 x 1 case masked: no row counts, exactly 0
        assert float(bound.max()) == 0.0 and not got_p.any() and (drop or n == 1)
    else:
        assert float(ref_p.abs().max()) > 0
        _note("front end alone: |d proj_in.[weight | bias] - fp64| / bound", _ratio(err, bound))
        _note("front end alone: relative L2 of d proj_in.weight", R.rel_l2(got["proj_in.weight"], ref_w))
        _note("front end alone: relative L2 of d proj_in.bias", R.rel_l2(got["proj_in.bias"], ref_b))


def test_front_end_every_row_masked_gives_exact_zeros():
    from voicebox_pytorch_amd.duration import _FrontEndFn

    case = dict(C.given_case(100, 32, 3, 17, False))
    case["cond_mask"] = torch.ones_like(case["cond_mask"])
    dp = _module(case["state"], 32, 100)
    cond, ids, _, cmask, dr, _, am8 = dp._resolve(case["cond"], case["ids"], case["cond_mask"], 0.0, None)
    conv = dp.conv_embed.dw_conv1d[0]
    x, _ = _FrontEndFn.apply(dp, ids, cond, cmask, dr, am8, False, dp.to_phoneme_emb.weight, dp.to_embed.weight, dp.to_embed.bias,
                             conv.weight, conv.bias, dp.proj_in.weight, dp.proj_in.bias)
    x.backward(torch.randn(3, 17, 64, generator=torch.Generator().manual_seed(0)).to(dev))
    assert dp.proj_in.weight.grad is not None and not dp.proj_in.weight.grad.any() and not dp.proj_in.bias.grad.any()
    assert float(dp.to_embed.weight.grad.abs().max()) > 0


# ----------------------------------------------------------------------------- 4: the module, both training branches
def _log(title, loss, ref, figures):
    proj = {k: v for k, v in figures.items() if k.startswith("proj_in.")}
    rest = {k: v for k, v in figures.items() if k != "loss" and not k.startswith(("proj_in.", "aligner."))}
    line = (f"{title}: loss {float(loss):.6f} vs {float(ref):.6f} (rel {figures['loss']:.2e}); gradients, relative L2: "
            + ", ".join(f"{k} {v:.3e}" for k, v in sorted(proj.items())) + f"; worst other {max(rest.values()):.3e}")
    print(line)
    LINES.append(line)
    _note("module cases, worst relative loss distance", figures["loss"])
    for k, v in proj.items():
        _note(f"module cases, worst distance of d {k}", v)
    _note("module cases, worst relative L2 over the other tensors", max(rest.values()))


@pytest.mark.parametrize("E,B,n,drop", R.GIVEN_CASES, ids=[f"E{E}_{B}x{n}_drop{int(d)}" for E, B, n, d in R.GIVEN_CASES])
def test_given_durations_loss_and_gradients(E, B, n, drop):
    case, ref = C.given_case(100, E, B, n, drop), C.given_reference(100, E, B, n, drop)
    assert R.margin(ref["d"], case["target"]) >= 0.5 - 1e-9
    dp = _module(case["state"], E, 100)
    args = dict(cond=case["cond"].to(dev), phoneme_ids=case["ids"].to(dev), target=case["target"].to(dev),
                cond_mask=case["cond_mask"].to(dev), cond_drop_prob=1.0 if drop else 0.0)
    loss = dp(**args)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "cuda"
    loss.backward()
    got = dict(loss=loss.detach().cpu(), grads=_grads(dp))
    assert dp.null_cond.grad is None
    assert got["grads"]["proj_in.weight"] is not None and got["grads"]["proj_in.bias"] is not None
    assert got["grads"]["proj_in.weight"].shape == (64, 100) and got["grads"]["proj_in.bias"].shape == (64,)
    assert all(v is not None for v in got["grads"].values())
    problems, figures = R.compare(got, ref)
    _log(f"given durations L=100 E={E} {B}x{n} cond_drop_prob={int(drop)}", loss, ref["loss"], figures)
    assert problems == [], (problems, figures)
    assert R.grad_tol("proj_in.weight") == R.GRAD_TOL and R.grad_tol("proj_in.bias") == R.GRAD_TOL  # in front of the stack
    if drop:
        assert not got["grads"]["proj_in.weight"].any() and not got["grads"]["proj_in.bias"].any()
    torch.manual_seed(0)
    a = dp(**args)
    torch.manual_seed(0)
    assert torch.equal(a, dp(**args)) and torch.equal(a, loss.detach())


@pytest.mark.parametrize("B,n,drop", [(3, 17, False), (2, 65, False), (2, 65, True)])
def test_everything_behind_the_pack_equals_the_codec_free_path(B, n, drop):
    """The codec-free predictor fed the projected rows the pack kernel wrote (its fp16 values, as fp32) reads the same to_embed
    operand bit for bit, so the loss and the gradient of every parameter the two predictors share are the same bits: proj_in adds
    two gradients and changes no other.  One exception by construction: columns E: of d to_embed.weight multiply the bf16 copy of the
    operand, which the fused pack rounds once from the fp32 sum and the codec-free pack from the fp16 value it was handed; those
    columns are held per element by test_front_end_node_alone."""
    case = C.given_case(100, 32, B, n, drop)
    fused = _module(case["state"], 32, 100)
    cond, ids, _, _, _, _, _ = fused._resolve(case["cond"], case["ids"], case["cond_mask"], 0.0, None)
    pw16, pb32 = fused._proj_operands()
    dev16 = torch.empty(B * n, 32 + 64, dtype=torch.float16, device=dev)
    L_.call("vbx_pack_phoneme_latent", ids, fused.to_phoneme_emb.weight.detach(), 32, cond, n, 100, pw16, pb32, None, None, None, dev16, B, n, 64, st())
    projected = dev16[:, 32:].reshape(B, n, 64).float()
    plain = _module({k: v for k, v in case["state"].items() if not k.startswith("proj_in.")}, 32)
    kw = dict(phoneme_ids=case["ids"].to(dev), target=case["target"].to(dev), cond_mask=case["cond_mask"].to(dev), cond_drop_prob=1.0 if drop else 0.0)
    la, lb = fused(cond=case["cond"].to(dev), **kw), plain(cond=projected, **kw)
    la.backward()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach())
    ga, gb = _grads(fused), _grads(plain)
    assert set(ga) == set(gb) | {"proj_in.weight", "proj_in.bias"}
    different = [k for k in gb if k != "to_embed.weight" and not torch.equal(ga[k], gb[k])]
    assert different == [], different
    assert torch.equal(ga["to_embed.weight"][:, :32], gb["to_embed.weight"][:, :32])


@pytest.mark.parametrize("flag", [False, True], ids=["l1_only", "with_align_loss"])
def test_aligner_branch(flag):
    E = 24
    case = C.aligner_case(100, E, flag=flag)
    al = case["aligner"]
    B, n = case["ids"].shape
    T = al["mel"].shape[1]
    dp = _module(case["state"], E, 100, aligner_state=al["state"])
    ids, mel = case["ids"].to(dev), al["mel"].to(dev)
    pmask = aligner_ref.mask_of(al["klens"], n)[:, None].to(torch.int32).to(dev)
    mmask = aligner_ref.mask_of(al["qlens"], T)[:, None].to(torch.int32).to(dev)
    plen, mlen = torch.tensor(al["klens"], device=dev), torch.tensor(al["qlens"], device=dev)
    with torch.no_grad():  # teacher-forced with the device's own hard alignment, as tests/test_duration_train_gpu.py does
        hard, soft, _, _ = dp.forward_aligner(dp.to_phoneme_emb.weight[ids.clamp(min=0)], pmask, mel, mmask)
    want = align_ref.maximum_path_batch_ref(soft.transpose(1, 2).cpu().double(), al["qlens"], al["klens"])[1]
    assert torch.equal(hard.cpu(), want.float())
    tf = dict(case, aligner=dict(al, durations=hard.cpu()))
    ref = C.reference(tf)
    assert float((ref["d"] - 2.5).abs().max()) <= 0.1 and float((ref["d"] - ref["target"]).abs().min()) >= 0.4
    loss = dp(cond=case["cond"].to(dev), phoneme_ids=ids, cond_mask=case["cond_mask"].to(dev), mel=mel, phoneme_len=plen, mel_len=mlen,
              phoneme_mask=pmask, mel_mask=mmask, return_aligned_phoneme_ids=flag)
    loss.backward()
    got = dict(loss=loss.detach().cpu(), grads=_grads(dp))
    assert got["grads"]["proj_in.weight"] is not None and float(got["grads"]["proj_in.weight"].abs().max()) > 0
    problems, figures = R.compare(got, ref, aligner_tol=aligner_ref.tolerance())
    _log(f"aligner branch L=100 E={E} {B}x{n} T={T} return_aligned_phoneme_ids={flag}", loss, ref["loss"], figures)
    assert problems == [], problems
    assert all((p.grad is not None) == flag for p in dp.aligner.parameters())


# ----------------------------------------------------------------------------- 5: latent_dim == dim
def test_latent_dim_equal_to_dim_is_the_codec_free_path():
    case = R.given_case(32, 3, 17, False)
    args = dict(cond=case["cond"].to(dev), phoneme_ids=case["ids"].to(dev), cond_mask=case["cond_mask"].to(dev))
    outs = []
    for attach in (False, True):
        dp = _module(case["state"], 32, 64 if attach else None)
        assert isinstance(dp.proj_in, torch.nn.Identity) and (dp.audio_enc_dec is not None) == attach
        dp.eval()
        d = dp(**args)
        dn = dp(cond_drop_prob=1.0, **args)
        dp.train()
        loss = dp(target=case["target"].to(dev), **args)
        loss.backward()
        outs.append((d, dn, loss.detach(), _grads(dp)))
    (d0, n0, l0, g0), (d1, n1, l1, g1) = outs
    assert torch.equal(d0, d1) and torch.equal(n0, n1) and torch.equal(l0, l1)
    assert list(g0) == list(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)


# ----------------------------------------------------------------------------- 6: wave -> phonemes -> sample
def test_end_to_end_sample_from_a_wave(golden):
    """small_codec_text's VoiceBox (latent 128 into dim 64, text-conditioned) with the fixture's predictor over the same codec"""
    from voicebox_pytorch_amd.sample_lens import length_regulate_restated

    g, c = golden("small_codec_text"), C.fixture_cases(golden("duration_codec"))["latent128_long_cond"]
    codec = ToyCodec(g["latent_dim"])
    assert g["latent_dim"] == c["latent_dim"] == 128

    def build(attach):
        vb = vbx.VoiceBox(dim=64, audio_enc_dec=codec, depth=2, dim_head=64, heads=2, time_hidden_dim=g["time_hidden_dim"],
                          ff_mult=g["ff_mult"], num_cond_tokens=50, dim_cond_emb=48, condition_on_text=True)
        vb.load_state_dict(g["state"], strict=False)
        dp = vbx.DurationPredictor(**KW)
        if attach:
            dp.attach_codec(codec)
        dp.load_state_dict({k: v for k, v in c["state"].items() if attach or not k.startswith("proj_in.")}, strict=False)
        return vbx.ConditionalFlowMatcherWrapper(voicebox=vb, duration_predictor=dp).to(dev)

    cfm = build(True)
    assert "duration_predictor.proj_in.weight" in cfm.state_dict()
    S = c["cond"].shape[1]
    wave = torch.randn(3, S * codec.hop, generator=torch.Generator().manual_seed(2)).to(dev)
    lat = codec.encode(wave)
    assert lat.shape == (3, S, 128)
    raw = c["ids"].to(dev)  # -1 padding on two rows
    ids = raw.clamp(min=0)
    draws = dict(coin=True, frac_lengths=torch.tensor([0.3, 0.6, 0.9]), rand=torch.tensor([0.1, 0.5, 0.8]))
    with rng_override(**draws):
        dur, aligned = cfm.duration_predictor.eval().forward_with_cond_scale(cond=lat, phoneme_ids=ids, return_aligned_phoneme_ids=True)
    n = aligned.shape[-1]
    assert n == int(dur.clamp(min=1).int().sum(-1).max())
    y0 = torch.randn(3, n, 128, generator=torch.Generator().manual_seed(1))
    with rng_override(y0=y0, **draws):
        from_wave = cfm.sample(cond=wave, phoneme_ids=ids, steps=3)
    with rng_override(y0=y0, **draws):
        from_lat = cfm.sample(cond=lat, phoneme_ids=ids, steps=3)
    assert from_wave.shape == (3, n * codec.hop) and bool(torch.isfinite(from_wave).all()) and torch.equal(from_wave, from_lat)
    with rng_override(y0=y0):  # the same frames from the aligned ids directly
        assert torch.equal(cfm.sample(cond=lat, semantic_token_ids=aligned, steps=3), from_wave)
    # lens="durations": the length regulator on the device's own durations, padding phonemes without frames
    with rng_override(**draws):
        dur_raw = cfm.duration_predictor.forward_with_cond_scale(cond=lat, phoneme_ids=raw)
    want_ids, want_lens = length_regulate_restated(raw.cpu(), dur_raw.cpu())
    y1 = torch.randn(3, int(want_lens.max()), 128, generator=torch.Generator().manual_seed(3))
    with rng_override(y0=y1, **draws):
        out = cfm.sample(cond=wave, phoneme_ids=raw, steps=3, lens="durations", decode_to_audio=False)
    assert out.shape == (3, int(want_lens.max()), 128) and cfm.last_sample_lens.tolist() == want_lens.tolist()
    short = int(want_lens.argmin())
    assert int(want_lens.min()) < int(want_lens.max()) and not out[short, int(want_lens[short]):].any()
    # without attach_codec the same call stops at the width assertion, which names the way out
    plain = build(False)
    with pytest.raises(AssertionError, match="attach_codec"):
        plain.sample(cond=wave, phoneme_ids=ids, steps=3)


def test_zz_report():
    """not a check: the measured values (profiles/duration_codec_parity.txt)"""
    out = ["DurationPredictor over codec latents, MI355X: tests/test_duration_codec_gpu.py against tests/duration_codec_ref.py (fp64, GEMM "
           f"operand roundings emulated) and tests/golden/duration_codec.pt; bounds: loss {R.LOSS_TOL} relative, gradients {R.GRAD_TOL} "
           "relative L2 per tensor (to_pred.0.* tightened, duration_train_ref.TIGHTENED), the reference's d1 / d_null / d3 2e-2 / 2e-2 / 4e-2"]
    out += LINES + [f"largest over all cases -- {k}: {RECORD[k]:.4g}" for k in sorted(RECORD)]
    print("\n" + "\n".join(out))
    path = os.environ.get("VBX_DURATION_CODEC_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(out) + "\n")
