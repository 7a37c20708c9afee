"""Block metric, references and yardstick of the block-gradient tests (tests/test_block_grads_gpu.py judges the kernels with them,
tests/test_block_check_cpu.py shows on the CPU that a correct backward passes and planted faults do not).

One Frobenius norm per gradient tensor hides an error confined to a tile: one 16 x 64 block of a 615 x 512 gradient scaled by 1.3 moves
the tensor's relative error by 0.3 * sqrt(1 / 312) ~ 1.7 %, below every whole-tensor bound of tests/test_model_gpu.py.  So every gradient
tensor is viewed as rows x last dimension (a 1-D tensor is one row), cut into blocks of 16 rows x 64 columns with tails as they fall
(16: the smallest row group any kernel owns; 64: the slab and panel width of gemm5 and the wide tiles), and block b is measured as

    metric_b = |got - ref|_b / max(|ref|_b, 0.5 * RMS(ref) * sqrt(numel_b))

numel_b being the block's REAL element count: the floor is half a typical block's norm (the device of attn_check._ONE_HOT_FLOOR), it
keeps a block that is legitimately near zero from dividing by nothing, and a 3-row tensor gets a floor that fits its 3-row blocks.

REFERENCE: the fp64 autograd of oracle/restate.py under restate.emulate_fp16_operands() -- the function the HIP backward differentiates.

YARDSTICK (`bf16_backward`): a stand-in for the product's backward precision, built from the reference alone.  The same emulated oracle
with restate._op wrapped for the duration of a context manager: the forward is untouched, the gradient arriving at every operand point
is rounded to bf16 -- the backward GEMMs' bf16 operands and the bf16 dxb / dqkv copies (DESIGN.md "Precision contract": every backward
GEMM operand is bf16).  s_case is the largest metric_b of the stand-in (in fp64) against the reference over every tensor of the case,
S_case the largest whole-tensor relative error the same way; both are computed by the test on the case's own inputs.

BOUND: every block of every tensor within FACTOR * s_case, every tensor within FACTOR * S_case, FACTOR = 8.  The kernels round operand
classes the stand-in does not model (fp16 P, bf16 dS and dO, the bf16 q and k copies); the project's record for the same comparison at
a well-conditioned point is 1.5 % whole-tensor (dim 128, depth 6: test_standalone_transformer_unet_ragged_shape_vs_oracle), about 3 x
the stand-in's whole-tensor 0.4 - 0.5 %; 8 leaves 2.5 x over that for per-block scatter.  No figure here comes from a run of the
kernels.  CONDITION: s_case <= S_CASE_CAP = 0.0125, so no block bound exceeds 10 %; inputs that break it are changed, not the cap.

Inputs are well posed: depth 2 (a dx chain, a first and a last layer, the cross-layer overlap plan all exist) at the trained-regime
logits the suite already uses -- every q_norm.gamma / k_norm.gamma x 0.25 (logit std ~5).
"""
import contextlib
import time
from dataclasses import dataclass, field

import torch

from oracle import restate

BLOCK_ROWS, BLOCK_COLS = 16, 64
FACTOR = 8.0
S_CASE_CAP = 0.0125
Y_REL, LOSS_ABS = 5e-3, 2e-4  # the suite's forward bounds against the emulated oracle (tests/test_model_gpu.py)
HEADS, DIM_HEAD, REGISTERS, COND_DIM = 16, 64, 16, 64


# ----------------------------------------------------------------------------- metric
def as_rows(t):
    """rows x last dimension; a 1-D (or 0-D) tensor is one row."""
    t = t.detach().double().cpu()
    return t.reshape(1, -1) if t.ndim <= 1 else t.reshape(-1, t.shape[-1])


def _block_sumsq(m):
    r, c = m.shape
    nr, nc = -(-r // BLOCK_ROWS), -(-c // BLOCK_COLS)
    p = torch.zeros(nr * BLOCK_ROWS, nc * BLOCK_COLS, dtype=torch.float64)
    p[:r, :c] = m
    return (p * p).reshape(nr, BLOCK_ROWS, nc, BLOCK_COLS).sum(dim=(1, 3))


def block_numel(r, c):
    rows = torch.full((-(-r // BLOCK_ROWS),), float(BLOCK_ROWS), dtype=torch.float64)
    cols = torch.full((-(-c // BLOCK_COLS),), float(BLOCK_COLS), dtype=torch.float64)
    rows[-1], cols[-1] = r - (len(rows) - 1) * BLOCK_ROWS, c - (len(cols) - 1) * BLOCK_COLS
    return rows[:, None] * cols[None, :]


@dataclass
class TensorErr:
    blocks: torch.Tensor  # metric_b, [row blocks, column blocks]
    whole: float          # relative L2 error of the whole tensor

    @property
    def worst(self):
        return float(self.blocks.max())

    @property
    def where(self):
        i = int(self.blocks.argmax())
        return i // self.blocks.shape[1], i % self.blocks.shape[1]


def tensor_err(got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    g, r = as_rows(got), as_rows(ref)
    assert bool(torch.isfinite(g).all()), "non-finite gradient"
    err, refn = _block_sumsq(g - r).sqrt(), _block_sumsq(r).sqrt()
    total = float(r.norm())
    rms = total / r.numel() ** 0.5
    den = torch.maximum(refn, 0.5 * rms * block_numel(*r.shape).sqrt())
    # a reference that is exactly zero everywhere: any non-zero element is an infinite error, zero is none
    blocks = torch.where(den > 0, err / den.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    whole = float((g - r).norm()) / total if total > 0 else (float("inf") if float(g.norm()) > 0 else 0.0)
    return TensorErr(blocks, whole)


def errors(got, ref):
    """{name: TensorErr} over every tensor of the reference; `got` must hold them all."""
    missing = [k for k in ref if k not in got or got[k] is None]
    assert not missing, f"no gradient for {missing}"
    return {k: tensor_err(got[k], ref[k]) for k in ref}


def yardstick(standin, ref):
    """(s_case, S_case): the stand-in's largest block metric and largest whole-tensor error against the reference."""
    e = errors(standin, ref)
    return max(v.worst for v in e.values()), max(v.whole for v in e.values())


CLASSES = ("to_qkv", "to_out", "ff.0", "ff.3", "adaLN weights", "adaLN biases", "gammas", "registers", "x", "cond", "embed", "head")


def tensor_class(name):
    if name in ("x", "cond"):
        return name
    if "to_qkv." in name:
        return "to_qkv"
    if "to_out." in name:
        return "to_out"
    if ".5.0." in name:
        return "ff.0"
    if ".5.3." in name:
        return "ff.3"
    if ".to_gamma." in name or ".to_beta." in name or name.endswith(".adaln_w"):
        return "adaLN weights" if name.endswith("weight") or name.endswith(".adaln_w") else "adaLN biases"
    if name.endswith("gamma"):
        return "gammas"
    if "register_tokens" in name:
        return "registers"
    if name.startswith("to_pred"):
        return "head"
    assert name.startswith(("to_embed", "conv_embed", "sinu_pos_emb")), name
    return "embed"


def report(label, errs, s_case, S_case):
    """The lines of profiles/block_grad_parity.txt: per tensor class the worst block and the worst whole-tensor error as ratios to
    their bounds, and the block that held the maximum."""
    lines = [f"{label}: s_case {s_case:.5f} S_case {S_case:.5f} (block bound {FACTOR * s_case:.4f}, whole-tensor bound {FACTOR * S_case:.4f})"]
    for c in CLASSES:
        mine = {k: v for k, v in errs.items() if tensor_class(k) == c}
        if not mine:
            continue
        kb = max(mine, key=lambda k: mine[k].worst)
        kw = max(mine, key=lambda k: mine[k].whole)
        lines.append(f"  {c:14s} block {mine[kb].worst / (FACTOR * s_case):.3f} of bound at {kb} block {mine[kb].where} of "
                     f"{tuple(mine[kb].blocks.shape)}; whole {mine[kw].whole / (FACTOR * S_case):.3f} of bound at {kw}")
    return lines


def violations(errs, s_case, S_case):
    """[(kind, tensor, block or None, value, bound)] of everything outside the bounds."""
    out = []
    for k, v in errs.items():
        if not v.worst <= FACTOR * s_case:
            out.append(("block", k, v.where, v.worst, FACTOR * s_case))
        if not v.whole <= FACTOR * S_case:
            out.append(("whole", k, None, v.whole, FACTOR * S_case))
    return out


def check(label, errs, s_case, S_case, verbose=True):
    lines = report(label, errs, s_case, S_case)
    if verbose:
        print("\n".join(lines))
    assert s_case <= S_CASE_CAP, (label, "the inputs break the condition s_case <= 0.0125: change the inputs, not the cap", s_case)
    bad = violations(errs, s_case, S_case)
    assert not bad, (label, sorted(bad, key=lambda b: -b[3] / b[4])[:8])
    return lines


# ----------------------------------------------------------------------------- yardstick
_ROUND = {"on": True}  # off: the rounding points pass the gradient through untouched (`reference` back-propagates one graph both ways)


class _Bf16Grad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype) if _ROUND["on"] else g


@contextlib.contextmanager
def bf16_backward():
    """restate._op as it is in the forward; the gradient arriving at every operand point is rounded to bf16 (a graph built inside keeps
    its rounding points after the context ends)."""
    orig = restate._op

    def op(x, tag=None, prescale=None):
        y = orig(x, tag, prescale)
        return _Bf16Grad.apply(y) if y.requires_grad else y

    restate._op = op
    try:
        yield
    finally:
        restate._op = orig


# ----------------------------------------------------------------------------- cases and references
@dataclass(frozen=True)
class Case:
    path: str   # "stack": vbx.Transformer, loss (y * dout).sum(); "model": VoiceBox in ConditionalFlowMatcherWrapper
    dim: int
    B: int
    N: int
    masked: bool
    seed: int = 21
    t: dict = field(default_factory=dict, compare=False, repr=False)  # state, inputs (built once by `inputs`)

    @property
    def name(self):
        return f"{self.path}-dim{self.dim}-{self.B}x{self.N}" + ("-masked" if self.masked else "")

    @property
    def cfg(self):
        return restate.Cfg(dim=self.dim, depth=2, heads=HEADS, dim_head=DIM_HEAD, num_register_tokens=REGISTERS, qk_norm=True)


def key_padding_mask(B, N):
    """drops the last fifth of the last batch row"""
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[-1, N - N // 5:] = False
    return mask


def stack_module(dim):
    import voicebox_pytorch_amd as vbx

    return vbx.Transformer(dim=dim, depth=2, heads=HEADS, dim_head=DIM_HEAD, num_register_tokens=REGISTERS, adaptive_rmsnorm=True,
                           adaptive_rmsnorm_cond_dim_in=COND_DIM, attn_qk_norm=True)


def inputs(case):
    """The case's weights and inputs as fp32 CPU tensors, the same on every call (its own generator state, the global one untouched)."""
    if case.t:
        return case.t
    t = {}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(case.seed)
        if case.path == "stack":
            # the recipe of test_standalone_transformer_unet_ragged_shape_vs_oracle: the module's own init, adaLN projections + 0.05 randn,
            # qk-norm gammas x 0.25
            tr = stack_module(case.dim)
            with torch.no_grad():
                for n, prm in tr.named_parameters():
                    if ".to_gamma." in n or ".to_beta." in n:
                        prm.add_(torch.randn_like(prm) * 0.05)
                    if "q_norm.gamma" in n or "k_norm.gamma" in n:
                        prm.mul_(0.25)
            t["state"] = {k: v.detach().clone() for k, v in tr.state_dict().items()}
            t["x"] = torch.randn(case.B, case.N, case.dim)
            t["cond"] = torch.randn(case.B, COND_DIM)
            t["dout"] = torch.randn(case.B, case.N, case.dim)
        else:
            state = restate.init_state_dict(case.cfg, case.seed)
            t["state"] = {k: (v * 0.25 if k.endswith("q_norm.gamma") or k.endswith("k_norm.gamma") else v) for k, v in state.items()}
            t["x1"], t["x0"] = torch.randn(case.B, case.N, case.dim), torch.randn(case.B, case.N, case.dim)
            t["times"], t["frac"], t["rand"] = torch.rand(case.B), 0.7 + 0.3 * torch.rand(case.B), torch.rand(case.B)
    t["mask"] = key_padding_mask(case.B, case.N) if case.masked else None
    case.t.update(t)
    return case.t


def _graph(case, dtype, standin):
    """(forward, scalar loss, {name: leaf}) of the emulated-precision oracle in `dtype`; standin: built inside bf16_backward()."""
    t = inputs(case)
    ctx = bf16_backward() if standin else contextlib.nullcontext()
    with ctx, restate.emulate_fp16_operands():
        if case.path == "stack":
            p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in t["state"].items() if v.is_floating_point()}
            p["x"], p["cond"] = t["x"].to(dtype).clone().requires_grad_(True), t["cond"].to(dtype).clone().requires_grad_(True)
            state = {k: v for k, v in p.items() if k not in ("x", "cond")}
            out = restate.transformer(p["x"], state, case.cfg, mask=t["mask"], cond=p["cond"], pre="")
            loss = (out * t["dout"].to(dtype)).sum()
        else:
            state = {k: v.to(dtype).clone().requires_grad_(v.is_floating_point() and k != "null_cond") for k, v in t["state"].items()}
            p = {k: v for k, v in state.items() if v.requires_grad}
            out = loss = restate.cfm_loss(state, case.cfg, t["x1"].to(dtype), t["x0"].to(dtype), t["times"].to(dtype), t["frac"], t["rand"],
                                          mask=t["mask"])
    return out.detach(), loss, p


def _backward(loss, leaves, keep=False):
    """{name: gradient} of the leaves the loss depends on"""
    grads = torch.autograd.grad(loss, list(leaves.values()), retain_graph=keep, allow_unused=True)
    return {k: g for k, g in zip(leaves, grads) if g is not None}


def oracle_grads(case, dtype=torch.float64, standin=False):
    """(forward, {name: gradient}) of the emulated-precision oracle in `dtype`; standin: with bf16_backward().  forward is y on the
    stack path and the loss on the model path; the stack path's gradients include "x" and "cond"."""
    out, loss, leaves = _graph(case, dtype, standin)
    return out, _backward(loss, leaves)


def loss32_emulated(case):
    """The loss the kernels are held to: the emulation in fp32, the arithmetic they accumulate in (emulated_oracle_grads)."""
    t = inputs(case)
    with torch.no_grad(), restate.emulate_fp16_operands():
        return float(restate.cfm_loss(t["state"], case.cfg, t["x1"], t["x0"], t["times"], t["frac"], t["rand"], mask=t["mask"]))


@dataclass
class Reference:
    forward: torch.Tensor  # y (stack) or the fp64 loss (model)
    grads: dict
    s_case: float
    S_case: float
    seconds: float         # CPU time of the oracle and the stand-in pass


def reference(case):
    """fp64 reference and the yardstick of a case; the callers cache it (functools.lru_cache) and leave it unchanged.  The stand-in's
    forward IS the reference's, so one graph is built and back-propagated twice: with the rounding points passing the gradient through
    (bit for bit the plain oracle's backward: tests/test_block_check_cpu.py) and with them rounding."""
    t0 = time.perf_counter()
    fwd, loss, leaves = _graph(case, torch.float64, standin=True)
    _ROUND["on"] = False
    try:
        ref = _backward(loss, leaves, keep=True)
    finally:
        _ROUND["on"] = True
    standin = _backward(loss, leaves)
    s, S = yardstick(standin, ref)
    return Reference(fwd, ref, s, S, time.perf_counter() - t0)


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))
