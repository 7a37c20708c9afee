"""fp64 restatement of DurationPredictor training (voicebox_pytorch_amd/duration.py, csrc/duration.hip), the inputs and the one
comparison the CPU and GPU tests share, the bounds of include/vbx.h as functions, and a list of planted faults.

The loss is the reference's masked L1 (voicebox_pytorch.py:858-866) taken on the PREDICTED durations -- the reference writes it on
the hidden state, which only broadcasts at degenerate shapes -- so this branch is unpinned against the reference by construction and
this file is the yardstick: oracle.restate.duration_predictor_forward (differentiable; under emulate_fp16_operands() its GEMM
operands are rounded as the device's forward rounds them), the loss below, torch autograd.  The aligner branch goes through
tests/aligner_ref.py (the network) and tests/align_ref.py (the search and the forward-sum loss).

Of the planted faults, "den_clamp_1" (clamp(min=1) instead of clamp(min=1e-5)) cannot move any output: the mask is boolean, so a
denominator below 1 is 0, and then the numerator is 0 as well.  It stays in the list; tests/test_duration_train_cpu.py asserts
exactly that for it and that every other fault is seen."""
import functools

import torch

import align_ref
import aligner_ref
from oracle import restate

U24 = 2.0 ** -24
LOSS_TOL = 5e-3   # relative; the bound the eval path holds against the emulated-operand restatement (test_duration_predictor_golden)
GRAD_TOL = 0.15   # relative L2 per tensor; the bound test_standalone_transformer_golden holds for the stack this loss runs back through
TAU = 0.0005
FAULTS = ("hidden_mean", "mask_or", "mask_not", "no_den", "den_clamp_1", "batch_sum", "sign_reversed", "align_loss_always",
          "align_loss_never", "emb_one_consumer")
ALIGNER_FAULTS = ("align_loss_always", "align_loss_never", "emb_one_consumer")
INVISIBLE_FAULTS = ("den_clamp_1",)
NEW_STAGES = ("to_pred.", "to_embed.", "conv_embed.", "to_phoneme_emb.")


def cfg_of(qk_norm=True, dim=64, depth=2, heads=2):
    return restate.Cfg(dim=dim, depth=depth, heads=heads, dim_head=64, num_register_tokens=0, qk_norm=qk_norm)


# to_pred sits downstream of the stack: its gradients are the head kernel's fp32 sums over the device's own hidden state and measure far
# below GRAD_TOL, so they are held to twice the largest value measured over all 14 module cases on an MI355X
# (profiles/duration_train_parity.txt: weight 1.895e-3, bias 1.455e-7).  The front end's tensors inherit the stack's backward and
# measure up to 0.10, in the range of the stack's own: they keep GRAD_TOL.
TIGHTENED = {"to_pred.0.weight": 2 * 1.895e-3, "to_pred.0.bias": 2 * 1.455e-7}


def grad_tol(name):
    """relative L2 allowed for a parameter's gradient"""
    return TIGHTENED.get(name, GRAD_TOL)


# ----------------------------------------------------------------------------- the loss
def masked_l1(d, target, cond_mask, self_attn_mask, fault=None):
    """:851-866 on d [B, n]: loss_mask = cond_mask & self_attn_mask, masked rows 0, num / den.clamp(min=1e-5) per row, mean"""
    if fault == "mask_or":
        m = cond_mask | self_attn_mask
    elif fault == "mask_not":
        m = ~cond_mask & self_attn_mask
    else:
        m = cond_mask & self_attn_mask
    l = (d - target.to(d.dtype)).abs()
    if fault == "sign_reversed":  # the same value, the gradient of -|d - t|
        l = 2.0 * l.detach() - l
    l = l.masked_fill(~m, 0.0)
    num, den = l.sum(-1), m.sum(-1).to(d.dtype)
    if fault == "no_den":
        q = num
    else:
        q = num / den.clamp(min=1.0 if fault == "den_clamp_1" else 1e-5)
    return q.sum() if fault == "batch_sum" else q.mean()


def leaves(state):
    return {k: (v.double().clone().requires_grad_(k != "null_cond") if v.is_floating_point() else v) for k, v in state.items()}


def predict(p, cfg, case, fault=None):
    """the durations [B, n] of restate.duration_predictor_forward; under "hidden_mean" the mean of the hidden state instead"""
    if fault == "hidden_mean":
        p = dict(p)
        p["to_pred.0.weight"] = torch.full_like(p["to_pred.0.weight"], 1.0 / cfg.dim) + 0.0 * p["to_pred.0.weight"]
        p["to_pred.0.bias"] = 0.0 * p["to_pred.0.bias"]
    return restate.duration_predictor_forward(p, cfg, case["cond"].double(), case["ids"], case["cond_mask"],
                                              cond_drop_mask=case.get("drop"), self_attn_mask=case.get("self_attn_mask"))


def reference(case, fault=None, emulate=True):
    """case: dict(state, qk_norm, cond [B, n, dim], ids [B, n], cond_mask, drop (bool [B] or None), and target [B, n] OR
    aligner = dict(state, mel [B, T, dim_in], klens, qlens, flag, durations (teacher-forced [B, n], or None: the fp64 search))).
    -> dict(loss, l1, align, d, target, grads {name: fp64 tensor or None}) with aligner gradients under "aligner." names."""
    cfg = cfg_of(case.get("qk_norm", True))
    p = leaves(case["state"])
    sam = case.get("self_attn_mask")
    sam = case["ids"] != -1 if sam is None else sam
    if emulate:
        with restate.emulate_fp16_operands():
            d = predict(p, cfg, case, fault)
    else:
        d = predict(p, cfg, case, fault)
    al, align, ap = case.get("aligner"), None, {}
    if al is None:
        target = case["target"].double()
    else:
        ap = {n: al["state"][n].double().clone().requires_grad_() for n in aligner_ref.PARAMS}
        emb = p["to_phoneme_emb.weight"][case["ids"].clamp(min=0)]
        if fault == "emb_one_consumer":
            emb = emb.detach()
        K, T = emb.shape[1], al["mel"].shape[1]
        attn, lp = aligner_ref.forward(ap, al["mel"].double().transpose(1, 2), emb, aligner_ref.mask_of(al["klens"], K), TAU)
        if al.get("durations") is not None:
            target = al["durations"].double()
        else:
            target = align_ref.maximum_path_batch_ref(attn[:, 0].detach(), al["qlens"], al["klens"])[1].double()
        with_align = al["flag"]
        if fault == "align_loss_always":
            with_align = True
        elif fault == "align_loss_never":
            with_align = False
        if with_align:
            align = align_ref.forward_sum_ref(lp[:, 0], al["klens"], al["qlens"])
    l1 = masked_l1(d, target, case["cond_mask"], sam, fault)
    loss = l1 if align is None else l1 + align
    names = [k for k, v in p.items() if torch.is_tensor(v) and v.requires_grad] + ["aligner." + n for n in ap]
    tensors = [p[k] for k in names if not k.startswith("aligner.")] + list(ap.values())
    gs = torch.autograd.grad(loss, tensors, allow_unused=True)
    return dict(loss=loss.detach(), l1=l1.detach(), align=None if align is None else align.detach(), d=d.detach(), target=target,
                grads=dict(zip(names, gs)))


def front_end(p, case):
    """the first autograd node alone (:811-826), operand roundings as active: (x [B, n, D], e = to_embed's output, emb [B, n, E],
    packed = [emb | cond''] [B, n, E + D])"""
    ids = case["ids"]
    sam = ids != -1
    cond = case["cond"].double() * (~case["cond_mask"])[..., None]
    if case.get("drop") is not None:
        cond = torch.where(case["drop"][:, None, None], p["null_cond"].double(), cond)
    emb = p["to_phoneme_emb.weight"][ids.clamp(min=0)]
    packed = torch.cat((emb, restate.curtail_or_pad(cond, ids.shape[-1])), dim=-1)
    e = restate._op(packed) @ restate._op(p["to_embed.weight"]).t() + p["to_embed.bias"]
    x = restate.conv_pos_embed(e, p["conv_embed.dw_conv1d.0.weight"], p["conv_embed.dw_conv1d.0.bias"], sam) + e
    return x, e, emb, packed


U_BF16 = 2.0 ** -8  # 8 significant bits
BF16_PRODUCT = 2 * U_BF16 + 2.0 ** -12  # two bf16-rounded factors, (1 + u)^2 - 1, and the fp32 error of the factor computed on the device


def rel_l2(x, ref):
    return aligner_ref.rel_l2(x, ref)


ZERO_REF_FLOOR = 2.0 ** -8  # the unit roundoff of bf16, the operand format of the backward GEMMs


def compare(got, ref, aligner_tol=None):
    """The one comparison of both test files.  got / ref: dict(loss, grads {name: tensor or None}).  Returns (problems, figures):
    the loss within LOSS_TOL relative, the same parameters with a gradient on both sides (None on one side only is a problem: it
    says which consumers took part), every gradient within grad_tol(name) in relative L2 -- aligner.* within aligner_tol when
    given.  A reference gradient that is EXACTLY zero (q_norm / k_norm gamma at one token: softmax over one key passes nothing to
    q and k) has no relative distance; there the tensor's norm must stay within the tolerance times ZERO_REF_FLOOR times the norm
    of the whole reference gradient, i.e. rounding residue of the 16-bit backward and nothing more (figure: norm / that scale).
    `figures` maps "loss" and every name to its measured distance."""
    problems, figures = [], {}
    lg, lr = float(got["loss"]), float(ref["loss"])
    figures["loss"] = abs(lg - lr) / max(abs(lr), 1e-300)
    if not figures["loss"] < LOSS_TOL:
        problems.append(f"loss {lg} vs {lr}: {figures['loss']:.3e}")
    whole = float(torch.sqrt(sum(r.double().pow(2).sum() for r in ref["grads"].values() if r is not None)))
    for name in sorted(set(got["grads"]) | set(ref["grads"])):
        g, r = got["grads"].get(name), ref["grads"].get(name)
        if (g is None) != (r is None):
            problems.append(f"{name}: gradient {'missing' if g is None else 'present'}, the reference's is {'missing' if r is None else 'present'}")
            continue
        if g is None:
            continue
        tol = aligner_tol if (aligner_tol is not None and name.startswith("aligner.")) else grad_tol(name)
        g = g.detach().cpu().reshape(r.shape)
        if float(r.double().norm()) == 0.0 and whole > 0.0:
            figures[name] = float(g.double().norm()) / (ZERO_REF_FLOOR * whole)
        else:
            figures[name] = rel_l2(g, r)
        if not figures[name] < tol:
            problems.append(f"{name}: {figures[name]:.3e} >= {tol}")
    return problems, figures


# ----------------------------------------------------------------------------- models and inputs
def init_state(dim_phoneme_emb, seed, pred_weight_scale=None, pred_bias=None, vocab=37, **kw):
    """the state dict of a default-initialised DurationPredictor(dim 64, depth 2, heads 2) (CPU, no compute)"""
    import voicebox_pytorch_amd as vbx

    rng = torch.random.get_rng_state()
    torch.manual_seed(seed)
    dp = vbx.DurationPredictor(num_phoneme_tokens=vocab, dim_phoneme_emb=dim_phoneme_emb, dim=64, depth=2, dim_head=64, heads=2, **kw)
    torch.random.set_rng_state(rng)
    sd = {k: v.detach().clone() for k, v in dp.state_dict().items()}
    # null_cond is initialised to zeros, where "the sample was dropped" and "the condition was masked" are the same function
    sd["null_cond"] = torch.randn(sd["null_cond"].shape, generator=torch.Generator().manual_seed(seed + 1000))
    if pred_weight_scale is not None:
        sd["to_pred.0.weight"] *= pred_weight_scale
    if pred_bias is not None:
        sd["to_pred.0.bias"].fill_(pred_bias)
    return sd


def make_inputs(B, n, seed, vocab=37, dim=64):
    """cond, ids with ragged -1 padding (row 0 full) and repeated ids, an explicit cond_mask whose LAST row leaves loss_mask empty
    (when B > 1): cond_mask is true only on that row's padding"""
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, n, dim, generator=g)
    ids = torch.randint(0, vocab, (B, n), generator=g)
    lens = [n] + [max(1, n - 1 - (3 * b) % max(n - 1, 1)) for b in range(1, B)]
    for b, l in enumerate(lens):
        ids[b, l:] = -1
    cond_mask = torch.rand(B, n, generator=g) < 0.6
    cond_mask[0, 0] = True
    if B > 1:
        cond_mask[B - 1] = ids[B - 1] == -1
    return cond, ids, cond_mask


@functools.lru_cache(maxsize=None)
def given_case(E=32, B=3, n=17, drop=False):
    """a given-durations case: default-initialised model, make_inputs, targets planted around the restatement's own prediction
    (operand roundings emulated); the same object for every test that asks (do not modify it)"""
    state = init_state(E, seed=3)
    cond, ids, cond_mask = make_inputs(B, n, seed=4)
    case = dict(state=state, qk_norm=True, cond=cond, ids=ids, cond_mask=cond_mask, drop=torch.ones(B, dtype=torch.bool) if drop else None)
    with torch.no_grad(), restate.emulate_fp16_operands():
        d = predict({k: v.double() if v.is_floating_point() else v for k, v in state.items()}, cfg_of(), case)
    case["target"] = planted_targets(d)
    case["d_ref"] = d
    return case


@functools.lru_cache(maxsize=None)
def given_reference(E=32, B=3, n=17, drop=False):
    return reference(given_case(E, B, n, drop))


GIVEN_CASES = [(E, B, n, drop) for E in (32, 24) for B, n in ((3, 17), (2, 65), (1, 1)) for drop in (False, True)]


def planted_targets(d_ref):
    """t = round(d_ref + s), s cycling over -2, -1, 1, 2: every position at least 0.5 from a sign change of d - t"""
    s = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)[torch.arange(d_ref.numel()) % 4].reshape(d_ref.shape)
    return torch.round(d_ref.double() + s)


def margin(d, target):
    return float((d.double() - target.double()).abs().min())


# ----------------------------------------------------------------------------- the bounds of include/vbx.h
def rowdot_bound(hid, w, b):
    """|d - d64| <= (D + 2) u (sum |x w| + |b|) per row"""
    D = hid.shape[-1]
    return (D + 2) * U24 * ((hid.double().abs() * w.double().abs()).sum(-1) + abs(float(b)))


def loss64(d, t, m):
    """(loss, num, den) in fp64 from given durations d [B, n], targets and the uint8 / bool mask"""
    m = m.bool()
    l = ((d.double() - t.double()).abs() * m).sum(-1)
    den = m.sum(-1).double()
    return (l / den.clamp(min=1e-5)).mean(), l, den


def loss_bound(loss, B, n):
    return (n + B + 4) * U24 * abs(float(loss))


def head_bwd_ref(hid, w, d, t, m, gscale):
    """fp64 (g [B, n], dhid, dw, db, sum |terms| of dw [D], sum |terms| of db) with the signs of the given d"""
    B, n = d.shape
    den = m.bool().sum(-1).double().clamp(min=1e-5)
    g = float(gscale) * m.bool().double() * torch.sign(d.double() - t.double()) / (B * den)[:, None]
    dhid = g[..., None] * w.double()
    terms = g[..., None] * hid.double()
    return g, dhid, terms.sum((0, 1)), g.sum(), terms.abs().sum((0, 1)), g.abs().sum()


def table_grad_ref(ids, ga, gb, V):
    """fp64 (gtable [V, E], sum |terms| [V, E], count [V]) of the two consumers' gradients (either None)"""
    g = sum(x.double() for x in (ga, gb) if x is not None)
    idx = ids.clamp(min=0).reshape(-1)
    E = g.shape[-1]
    gt, ab = torch.zeros(V, E, dtype=torch.float64), torch.zeros(V, E, dtype=torch.float64)
    gt.index_add_(0, idx, g.reshape(-1, E))
    ab.index_add_(0, idx, g.reshape(-1, E).abs())
    return gt, ab, torch.bincount(idx, minlength=V)


# ----------------------------------------------------------------------------- the aligner case and the training run
ALIGNER_DIMS = dict(dim_in=16, attn_channels=8)


def aligner_case(dim_phoneme_emb=24, seed=5, flag=True, B=2, n=17, T=67):
    """2 x 17 phonemes against T = 67 mel frames: prefix masks, row 1 short in both; the mel follows aligner_ref.planted_path (frame
    t is a fixed random projection of the embedding of the phoneme the planted path puts it on, plus noise).  to_pred starts at
    weight x 0.01 and bias 2.5, so every prediction is within 0.1 of 2.5 and at least 0.4 from any integer target."""
    state = init_state(dim_phoneme_emb, seed, pred_weight_scale=0.01, pred_bias=2.5)
    g = torch.Generator().manual_seed(seed + 100)
    cond = torch.randn(B, n, 64, generator=g)
    ids = torch.randint(0, 37, (B, n), generator=g)
    klens, qlens = [n] + [n - 5] * (B - 1), [T] + [T - 13] * (B - 1)
    for b in range(B):
        ids[b, klens[b]:] = -1
    cond_mask = torch.rand(B, n, generator=g) < 0.7
    cond_mask[:, 0] = True
    path = aligner_ref.planted_path(klens, qlens, T, n)[:, 0].float()  # [B, T, K]
    proj = torch.randn(dim_phoneme_emb, ALIGNER_DIMS["dim_in"], generator=g) * dim_phoneme_emb ** -0.5
    emb = state["to_phoneme_emb.weight"][ids.clamp(min=0)]
    mel = path @ (emb @ proj) + 0.1 * torch.randn(B, T, ALIGNER_DIMS["dim_in"], generator=g)
    al = dict(state=aligner_ref.init_state(ALIGNER_DIMS["dim_in"], dim_phoneme_emb, ALIGNER_DIMS["attn_channels"], seed + 1, tau=TAU),
              mel=mel, klens=klens, qlens=qlens, flag=flag, durations=None)
    return dict(state=state, qk_norm=True, cond=cond, ids=ids, cond_mask=cond_mask, drop=None, aligner=al)


TRAIN_LR = 0.05   # chosen on the fp64 run below: 2.43 -> 0.22 (0.09 x) in 20 steps; 0.1 gives 0.06 x, 0.2 0.20 x (test_duration_train_cpu.py
                  # asserts the factor)
TRAIN_STEPS = 20


def train_case(seed=9):
    state = init_state(32, seed)
    cond, ids, cond_mask = make_inputs(3, 17, seed + 1)
    cond_mask = torch.ones_like(cond_mask)
    target = torch.full(ids.shape, 3.0)  # planted durations: three frames a phoneme
    return dict(state=state, qk_norm=True, cond=cond, ids=ids, cond_mask=cond_mask, drop=None, target=target)


def train_run_ref(case, lr=TRAIN_LR, steps=TRAIN_STEPS):
    """Adam on the fp64 restatement (operand roundings emulated): the losses before step 0 .. after the last step"""
    cfg = cfg_of(case["qk_norm"])
    p = leaves(case["state"])
    params = [v for v in p.values() if torch.is_tensor(v) and v.requires_grad]
    opt = torch.optim.Adam(params, lr=lr)
    sam = case["ids"] != -1
    losses = []
    for step in range(steps + 1):
        with restate.emulate_fp16_operands():
            d = predict(p, cfg, case)
        loss = masked_l1(d, case["target"].double(), case["cond_mask"], sam)
        losses.append(float(loss.detach()))
        if step < steps:
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
    return losses
