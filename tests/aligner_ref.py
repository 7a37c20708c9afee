"""fp64 restatement of the Aligner network (voicebox_pytorch_amd.Aligner / aligner_attention; csrc/aligner.hip), forward AND a
hand-written backward, the inputs the CPU and GPU tests share, and the bounds of include/vbx.h as functions.  naturalspeech2_pytorch
is absent: parity with it is UNPINNED; the arithmetic is the convolutional attention of "One TTS Alignment To Rule Them All" /
RAD-TTS as the issue states it.

The convolutions are shifted matrix products, the attention a difference chunked over the query frames (so that the key limit fits
in memory), the backward the formulas the kernels implement -- tests/test_aligner_cpu.py holds all of it against an independent
construction from nn.Conv1d, the broadcast difference, softmax and autograd.  `fault=` plants a deliberately wrong variant, and
`emulate=True` rounds the GEMM operands (weights and layer inputs) as the device's forward does: to fp16 in the last layer of each
stack, to an fp16 hi + lo pair in the layers in front of a ReLU."""
import functools
import math

import torch
from torch import nn

import align_ref

U24 = 2.0 ** -24
FLT_MAX = float(torch.finfo(torch.float32).max)
QUERY, KEY = ("query_layers.0", "query_layers.2", "query_layers.4"), ("key_layers.0", "key_layers.2")
PARAMS = tuple(f"{l}.{p}" for l in QUERY + KEY for p in ("weight", "bias"))

FWD_FAULTS = ("no_relu", "taps_reversed", "pad_wrong_end", "temperature_sign", "mask_off_by_one", "softmax_axis", "logprob_masked")
BWD_FAULTS = ("no_factor_2", "dk_sign")
FAULTS = FWD_FAULTS + BWD_FAULTS


# ----------------------------------------------------------------------------- parameters
def shapes_of(dim_in, dim_hidden, attn):
    return {"key_layers.0.weight": (2 * dim_hidden, dim_hidden, 3), "key_layers.0.bias": (2 * dim_hidden,),
            "key_layers.2.weight": (attn, 2 * dim_hidden, 1), "key_layers.2.bias": (attn,),
            "query_layers.0.weight": (2 * dim_in, dim_in, 3), "query_layers.0.bias": (2 * dim_in,),
            "query_layers.2.weight": (dim_in, 2 * dim_in, 1), "query_layers.2.bias": (dim_in,),
            "query_layers.4.weight": (attn, dim_in, 1), "query_layers.4.bias": (attn,)}


def torch_module(dim_in, dim_hidden, attn):
    """the network from torch's own layers (nn.Conv1d's default initialisation): the independent construction"""
    m = nn.Module()
    m.key_layers = nn.Sequential(nn.Conv1d(dim_hidden, 2 * dim_hidden, 3, padding=1), nn.ReLU(), nn.Conv1d(2 * dim_hidden, attn, 1))
    m.query_layers = nn.Sequential(nn.Conv1d(dim_in, 2 * dim_in, 3, padding=1), nn.ReLU(), nn.Conv1d(2 * dim_in, dim_in, 1), nn.ReLU(),
                                   nn.Conv1d(dim_in, attn, 1))
    return m


def torch_forward(m, queries, keys, mask, tau):
    """naturalspeech2_pytorch's Aligner.forward, from its pieces: (attn, attn_logprob) [B, 1, T, K]"""
    k = m.key_layers(keys.transpose(1, 2))
    q = m.query_layers(queries)
    a = -tau * ((q[:, :, :, None] - k[:, :, None]) ** 2).sum(1, keepdim=True)
    logprob = a.clone()
    if mask is not None:
        a = a.masked_fill(~mask.reshape(mask.shape[0], 1, 1, -1).bool(), -torch.finfo(a.dtype).max)
    return torch.softmax(a, 3), logprob


def init_state(dim_in, dim_hidden, attn, seed, tau=0.0005, target_std=2.0, T=48, K=24):
    """Default initialisation, then the last layer of each stack scaled so that attn_logprob has a standard deviation over the keys
    of about target_std on random inputs (a trained regime; at the raw initialisation the map is flat and nothing is tested)."""
    g = torch.Generator().manual_seed(seed)
    rng = torch.random.get_rng_state()
    torch.manual_seed(seed)
    m = torch_module(dim_in, dim_hidden, attn)
    torch.random.set_rng_state(rng)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    q, k = torch.randn(2, dim_in, T, generator=g), torch.randn(2, K, dim_hidden, generator=g)
    lp = forward(sd, q, k, None, tau)[1]
    s = float(lp.std(3).mean())
    gain = math.sqrt(target_std / max(s, 1e-30))  # logprob is quadratic in the encodings
    for name in ("query_layers.4", "key_layers.2"):
        sd[name + ".weight"] *= gain
        sd[name + ".bias"] *= gain
    return sd


def make_inputs(B, T, K, dim_in, dim_hidden, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, dim_in, T, generator=g), torch.randn(B, K, dim_hidden, generator=g)


def lengths(B, T, K, variant=0):
    """per row (key_len, query_len): kind (b + variant) % 3 = full, short, fully masked"""
    kl, ql = [], []
    for b in range(B):
        kind = (b + variant) % 3
        k = K if kind == 0 else (max(1, (2 * K) // 3) if kind == 1 else 0)
        q = T if kind != 1 else max(1, T - T // 5)
        kl.append(k)
        ql.append(q)
    return kl, ql


def variants(B):
    return list(range((3 + B - 1) // B)) if B < 3 else [0]


def mask_of(klens, K):
    return torch.arange(K)[None, :] < torch.tensor(klens)[:, None]


def planted_path(klens, qlens, T, K):
    """a fixed 0 / 1 map [B, 1, T, K] from the lengths (frame t on key floor(t k / q)): the target of the binarisation term.  Data
    of the test, the same for the device and the restatement; also where q < k (the forward-sum loss is 0 there, this term is
    not); zero on rows without keys."""
    p = torch.zeros(len(klens), 1, T, K, dtype=torch.float64)
    for b, (k, q) in enumerate(zip(klens, qlens)):
        if k >= 1 and q >= 1:
            t = torch.arange(q)
            p[b, 0, t, (t * k) // q] = 1.0
    return p


# ----------------------------------------------------------------------------- forward
def _shift(x, s):
    """y[:, t] = x[:, t + s], zero outside"""
    if s == 0:
        return x
    T = x.shape[1]
    z = torch.zeros_like(x)
    if abs(s) >= T:
        return z
    if s > 0:
        z[:, :T - s] = x[:, s:]
    else:
        z[:, -s:] = x[:, :T + s]
    return z


def _r16(x, emulate, pair):
    """the device's operand rounding: fp16, or (a layer in front of a ReLU) the fp16 hi + lo pair"""
    if not emulate:
        return x
    hi = x.to(torch.float16).to(x.dtype)
    return hi + (x - hi).to(torch.float16).to(x.dtype) if pair else hi


def _offsets(taps, fault):
    if taps == 1:
        return [0]
    return [-2, -1, 0] if fault == "pad_wrong_end" else [-1, 0, 1]


def _conv(x, w, b, fault, emulate, pair=False):
    """x [B, T, Cin] -> [B, T, Cout]: sum_tap x(t + tap - 1) W[:, :, tap]^T + b"""
    taps = w.shape[2]
    y = b.expand(x.shape[0], x.shape[1], -1).clone()
    for tap, off in enumerate(_offsets(taps, fault)):
        wt = w[:, :, taps - 1 - tap] if fault == "taps_reversed" else w[:, :, tap]
        y = y + _shift(_r16(x, emulate, pair), off) @ _r16(wt, emulate, pair).t()
    return y


def _stack(x, sd, names, fault, emulate):
    """-> (encodings, [input of every layer], [pre-activation of every layer])"""
    ins, pres = [], []
    for i, n in enumerate(names):
        if i > 0 and fault != "no_relu":
            x = x.clamp(min=0)
        ins.append(x)
        x = _conv(x, sd[n + ".weight"], sd[n + ".bias"], fault, emulate, pair=i < len(names) - 1)
        pres.append(x)
    return x, ins, pres


def _chunks(T, K, A):
    step = max(1, (1 << 24) // max(1, K * A))
    return [(t, min(T, t + step)) for t in range(0, T, step)]


def attention(q, k, mask, tau, fault=None):
    """q [B, T, A], k [B, K, A], mask bool [B, K] or None -> (attn, logprob) [B, 1, T, K] in q's dtype"""
    B, T, A = q.shape
    K = k.shape[1]
    if fault == "temperature_sign":
        tau = -tau
    lp = torch.cat([-tau * ((q[:, a:b, None, :] - k[:, None, :, :]) ** 2).sum(-1) for a, b in _chunks(T, K, A)], 1)
    x = lp
    if mask is not None:
        m = mask
        if fault == "mask_off_by_one":  # one key too many is kept
            m = mask | torch.cat((torch.zeros_like(mask[:, :1]), mask[:, :-1]), 1)
        x = lp.masked_fill(~m[:, None, :], -FLT_MAX)
    attn = torch.softmax(x, 1 if fault == "softmax_axis" else 2)
    if fault == "logprob_masked":
        lp = x
    return attn[:, None], lp[:, None]


def encode(sd, queries, keys, fault=None, emulate=False):
    sd = {n: v.to(queries.dtype) for n, v in sd.items()}
    q, qin, qpre = _stack(queries.transpose(1, 2), sd, QUERY, fault, emulate)
    k, kin, kpre = _stack(keys, sd, KEY, fault, emulate)
    return q, k, dict(sd=sd, qin=qin, qpre=qpre, kin=kin, kpre=kpre)


def forward(sd, queries, keys, mask, tau, fault=None, emulate=False, dtype=torch.float64, cache=False):
    """queries [B, dim_in, T], keys [B, K, dim_hidden], mask bool [B, K] or None -> (attn, attn_logprob) [B, 1, T, K] (, cache)"""
    q, k, c = encode(sd, queries.to(dtype), keys.to(dtype), fault, emulate)
    mask = None if mask is None else mask.reshape(mask.shape[0], -1).bool()
    attn, lp = attention(q, k, mask, tau, fault)
    if not cache:
        return attn, lp
    c.update(q=q, k=k, mask=mask, tau=tau, attn=attn)
    return attn, lp, c


# ----------------------------------------------------------------------------- backward, by hand
def attention_backward(q, k, mask, tau, attn, g_attn, g_logprob, fault=None):
    """-> (dq, dk, G): G = g_logprob + mask attn (g_attn - sum_j attn g_attn); dq_t = -2 tau sum_j G_tj (q_t - k_j);
    dk_j = +2 tau sum_t G_tj (q_t - k_j)"""
    B, T, A = q.shape
    K = k.shape[1]
    G = torch.zeros(B, T, K, dtype=q.dtype)
    if g_attn is not None:
        a, ga = attn[:, 0], g_attn[:, 0]
        G = a * (ga - (a * ga).sum(2, keepdim=True))
        if mask is not None:
            G = G * mask[:, None, :]
    if g_logprob is not None:
        G = G + g_logprob[:, 0]
    c = (1.0 if fault == "no_factor_2" else 2.0) * tau
    dq, dk = torch.zeros_like(q), torch.zeros_like(k)
    for a, b in _chunks(T, K, A):
        d = q[:, a:b, None, :] - k[:, None, :, :]
        gd = G[:, a:b, :, None] * d
        dq[:, a:b] = -c * gd.sum(2)
        dk += (-c if fault == "dk_sign" else c) * gd.sum(1)
    return dq, dk, G


def _stack_backward(g, sd, names, ins, pres):
    """g: gradient of the last pre-activation -> (gradient of the stack's input [B, T, Cin], {name: gradient})"""
    grads = {}
    for i in range(len(names) - 1, -1, -1):
        w = sd[names[i] + ".weight"]
        taps = w.shape[2]
        if i < len(names) - 1:
            g = g * (pres[i] > 0)
        grads[names[i] + ".bias"] = g.sum((0, 1))
        offs = _offsets(taps, None)
        grads[names[i] + ".weight"] = torch.stack([torch.einsum("bto,btc->oc", g, _shift(ins[i], off)) for off in offs], 2)
        g = sum(_shift(g @ w[:, :, tap], -off) for tap, off in enumerate(offs))
    return g, grads


def backward(c, g_attn, g_logprob, fault=None):
    """the cache of forward(..., cache=True) and the gradients of both maps (either may be None) -> {parameter name, "queries",
    "keys": gradient}"""
    dq, dk, _ = attention_backward(c["q"], c["k"], c["mask"], c["tau"], c["attn"], g_attn, g_logprob, fault)
    dxq, gq = _stack_backward(dq, c["sd"], QUERY, c["qin"], c["qpre"])
    dxk, gk = _stack_backward(dk, c["sd"], KEY, c["kin"], c["kpre"])
    return {**gq, **gk, "queries": dxq.transpose(1, 2), "keys": dxk}


# ----------------------------------------------------------------------------- the loss of the gradient tests
def loss_fn(attn, logprob, klens, qlens, path, fsl=None):
    """forward-sum loss on the log-probabilities plus a binarisation term on the soft map, -sum(path log attn) / sum(path)
    (naturalspeech2_pytorch's BinLoss against a given hard path).  fsl: the forward-sum implementation, default the fp64 one."""
    fs = align_ref.forward_sum_ref(logprob[:, 0], klens, qlens) if fsl is None else fsl(logprob)
    n = path.sum().clamp(min=1)
    return fs + -(torch.log(attn.clamp(min=1e-12)) * path.to(attn.dtype)).sum() / n


def loss_grads(attn, logprob, klens, qlens, path):
    """fp64: (loss, d loss / d attn, d loss / d logprob)"""
    a, l = attn.detach().clone().requires_grad_(), logprob.detach().clone().requires_grad_()
    loss = loss_fn(a, l, klens, qlens, path)
    ga, gl = torch.autograd.grad(loss, (a, l), allow_unused=True)
    return loss.detach(), (torch.zeros_like(a) if ga is None else ga), (torch.zeros_like(l) if gl is None else gl)


def reference_autograd(sd, queries, keys, klens, qlens, tau, fault=None, module=None):
    """the same by autograd through the restatement's forward -- or, with module (a torch_module in fp64), through torch's own
    layers"""
    K, T = keys.shape[1], queries.shape[2]
    mask = mask_of(klens, K)
    qx, kx = queries.double().requires_grad_(), keys.double().requires_grad_()
    if module is None:
        leaves = {n: sd[n].double().requires_grad_() for n in PARAMS}
        attn, lp = forward(leaves, qx, kx, mask, tau, fault=fault)
    else:
        leaves = dict(module.named_parameters())
        attn, lp = torch_forward(module, qx, kx, mask, tau)
    loss = loss_fn(attn, lp, klens, qlens, planted_path(klens, qlens, T, K))
    names = list(PARAMS) + ["queries", "keys"]
    tensors = [leaves[n] for n in PARAMS] + [qx, kx]
    gs = torch.autograd.grad(loss, tensors, allow_unused=True)
    grads = {n: (torch.zeros_like(t) if g is None else g) for n, t, g in zip(names, tensors, gs)}
    return dict(attn=attn.detach(), logprob=lp.detach(), loss=loss.detach(), grads=grads)


def reference(sd, queries, keys, klens, qlens, tau, fault=None, emulate=False):
    """everything the tests compare against for one case: dict(attn, logprob, loss, grads {name: fp64}).  The gradients come from
    the hand-written backward (which is where the backward faults live); a forward fault is differentiated by autograd, so that
    its gradient is the gradient of the faulty forward"""
    if fault in FWD_FAULTS:
        return reference_autograd(sd, queries, keys, klens, qlens, tau, fault=fault)
    K, T = keys.shape[1], queries.shape[2]
    mask = mask_of(klens, K)
    with torch.no_grad():
        attn, lp, c = forward(sd, queries, keys, mask, tau, fault=fault, emulate=emulate, cache=True)
    loss, ga, gl = loss_grads(attn, lp, klens, qlens, planted_path(klens, qlens, T, K))
    return dict(attn=attn, logprob=lp, loss=loss, grads=backward(c, ga, gl, fault))


# ----------------------------------------------------------------------------- measures and the tolerance of the GPU tests
def logprob_movement(x, ref):
    """max |x - ref| / RMS(ref)"""
    return float((x.double() - ref.double()).abs().max() / ref.double().pow(2).mean().sqrt().clamp(min=1e-300))


def rel_l2(x, ref):
    n = float(ref.double().norm())
    d = float((x.double() - ref.double()).norm())
    return d / n if n > 0 else (0.0 if d == 0 else math.inf)


def gradient_movement(grads, ref):
    """the largest per-tensor relative L2 distance"""
    return max(rel_l2(grads[n], ref[n]) for n in ref)


PLANT = dict(B=3, T=21, K=9, dim_in=16, dim_hidden=24, attn=8, tau=0.0005, seed=11)


@functools.lru_cache(maxsize=None)
def planted_movements():
    """{fault: (movement of attn_logprob, movement of the gradients)} on a small case with full, short and fully masked rows"""
    p = PLANT
    sd = init_state(p["dim_in"], p["dim_hidden"], p["attn"], p["seed"], p["tau"])
    queries, keys = make_inputs(p["B"], p["T"], p["K"], p["dim_in"], p["dim_hidden"], p["seed"] + 1)
    klens, qlens = lengths(p["B"], p["T"], p["K"])
    good = reference(sd, queries, keys, klens, qlens, p["tau"])
    out = {}
    for f in FAULTS:
        bad = reference(sd, queries, keys, klens, qlens, p["tau"], fault=f)
        out[f] = (logprob_movement(bad["logprob"], good["logprob"]), gradient_movement(bad["grads"], good["grads"]))
    return out


def tolerance():
    """What the GPU tests allow the module, for attn_logprob (max |error| / RMS) and for every gradient tensor (relative L2): a tenth
    of the smallest movement any planted fault makes in the measure it moves most.  Computed from the restatement alone."""
    return min(max(a, b) for a, b in planted_movements().values()) / 10.0


# ----------------------------------------------------------------------------- the bounds of include/vbx.h
def logprob_bound(ref, A):
    return (A + 4) * U24 * ref.abs()


def softmax_ref_and_bound(logprob, mask):
    """the fp64 masked softmax p of the kernel's own logprob [B, 1, T, K] (a masked key exactly 0, a fully masked row 1 / K) and the
    per-element bound (|x - m| + sum_j p_j |x_j - m| + ceil(K / 64) + 16) u p + 2^-126"""
    x = logprob.double()
    K = x.shape[3]
    if mask is not None:
        keep = mask.reshape(mask.shape[0], 1, 1, K).bool().expand_as(x)
        dead = ~keep.any(3, keepdim=True)
        keep = keep | dead  # every key filled alike: the plain softmax of equal values
        x = torch.where(dead, torch.zeros_like(x), x)
    else:
        keep = torch.ones_like(x, dtype=torch.bool)
    m = x.masked_fill(~keep, -math.inf).amax(3, keepdim=True)
    e = torch.where(keep, torch.exp(x - m), torch.zeros_like(x))
    p = e / e.sum(3, keepdim=True)
    dist = torch.where(keep, (x - m).abs(), torch.zeros_like(x))
    bound = (dist + (p * dist).sum(3, keepdim=True) + math.ceil(K / 64) + 16) * U24 * p + 2.0 ** -126
    return p, bound


def attn_grad_bounds(q, k, mask, tau, attn, g_attn, g_logprob):
    """(bound of dq, bound of dk): (n + 32) u 2 tau sum gh |q - k|, gh = |g_logprob| + attn (|g_attn| + sum_j attn |g_attn|)"""
    B, T, A = q.shape
    K = k.shape[1]
    gh = torch.zeros(B, T, K, dtype=torch.float64)
    if g_attn is not None:
        a, ga = attn[:, 0].double(), g_attn[:, 0].double().abs()
        gh = a * (ga + (a * ga).sum(2, keepdim=True))
    if g_logprob is not None:
        gh = gh + g_logprob[:, 0].double().abs()
    bq, bk = torch.zeros(B, T, A, dtype=torch.float64), torch.zeros(B, K, A, dtype=torch.float64)
    for a, b in _chunks(T, K, A):
        d = (q[:, a:b, None, :].double() - k[:, None, :, :].double()).abs() * gh[:, a:b, :, None]
        bq[:, a:b] = d.sum(2)
        bk += d.sum(1)
    return (K + 32) * U24 * 2 * tau * bq, (T + 32) * U24 * 2 * tau * bk


# ----------------------------------------------------------------------------- the direct-form contract, on the CPU in fp32
def sumsq_fp32(q, k, form="direct"):
    """sum_c (q_c - k_c)^2 of fp32 rows [n, A] as an fp32 chain in index order ("direct": torch.addcmul is not fused, so this is the
    multiply-then-add chain, whose bound is no better than the fmaf chain's), the expanded form |q|^2 + |k|^2 - 2 q.k, or the direct
    chain on operands rounded to fp16 once -- the two planted faults"""
    q, k = q.float(), k.float()
    if form == "fp16":
        q, k = q.half().float(), k.half().float()
    acc = torch.zeros(q.shape[0], dtype=torch.float32)
    if form == "expanded":
        qq, kk, qk = acc.clone(), acc.clone(), acc.clone()
        for c in range(q.shape[1]):
            qq = qq + q[:, c] * q[:, c]
            kk = kk + k[:, c] * k[:, c]
            qk = qk + q[:, c] * k[:, c]
        return qq + kk - 2 * qk
    for c in range(q.shape[1]):
        d = q[:, c] - k[:, c]
        acc = acc + d * d
    return acc
