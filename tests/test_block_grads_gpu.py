"""The backward of a whole transformer layer at the widths the benchmark trains (dim 512 and 1024, 16 heads of 64, 16 register tokens,
qk-norm, adaptive RMSNorm, the padded FeedForward width 1365 -> 1408 / 2730 -> 2752): every gradient tensor, block by block (16 rows x
64 columns), against the fp64 emulated-precision oracle.  tests/block_check.py has the metric, the references, the yardstick and the
bound (8 x the bf16-backward stand-in's own worst block / worst tensor on the case's inputs; no figure from a run of the kernels);
tests/test_block_check_cpu.py shows on the CPU that a correct backward passes and that planted tile faults do not.

Three ways into vbx_model_backward_layer: the standalone stack (vbx.Transformer: x and cond get gradients too), the model through
autograd (wrapper(x1).backward(): every parameter materialised) and the call TrainStep.step makes (adaLN weight gradients in factor
form, one deferred slab reduce for all layers).  Shapes: 3 x 189 frames with the last fifth of the last row padded (3 x 205 = 615 rows:
no multiple of 16, 64 or 128), 1 x 8 (every tile a tail), and the full-route shape 16 x 496 (8192 rows: every GEMM of the layer on the
kernel it gets at the benchmark's 8 x 1040 rows, asserted below).

With -s every case prints s_case / S_case and, per tensor class, the kernels' worst block and worst tensor as ratios to their bounds
(profiles/block_grad_parity.txt)."""
import functools

import pytest
import torch

import block_check as bc

pytestmark = pytest.mark.gpu
dev = "cuda"

FULL = (16, 496)      # 16 x (496 + 16) = 8192 rows
BENCH = (8, 1024)     # bench.py: 8 x (1024 + 16) = 8320 rows


@functools.lru_cache(maxsize=None)
def _reference(case):
    return bc.reference(case)


def _judge(case, got, label=None):
    r = _reference(case)
    errs = bc.errors(got, r.grads)
    label = label or case.name
    print(f"[block] {label}: fp64 oracle + stand-in {r.seconds:.1f} s of CPU time")
    for line in bc.report(label, errs, r.s_case, r.S_case):
        print("[block] " + line)
    bc.check(label, errs, r.s_case, r.S_case, verbose=False)


# ----------------------------------------------------------------------------- the standalone stack
@pytest.mark.parametrize("dim,B,N,masked", [(512, 3, 189, True), (1024, 3, 189, True), (512, 1, 8, False)])
def test_stack_block_grads(dim, B, N, masked):
    case = bc.Case("stack", dim, B, N, masked)
    t = bc.inputs(case)
    tr = bc.stack_module(dim)
    tr.load_state_dict(t["state"])
    tr = tr.to(dev)
    x, cond = t["x"].to(dev).requires_grad_(True), t["cond"].to(dev).requires_grad_(True)
    y = tr(x, mask=t["mask"].to(dev) if masked else None, adaptive_rmsnorm_cond=cond)
    (y * t["dout"].to(dev)).sum().backward()
    r = _reference(case)
    e_y = bc.rel(y, r.forward)
    print(f"[block] {case.name}: y vs emulated oracle {e_y:.2e}")
    assert e_y < bc.Y_REL, e_y
    got = {k: p.grad for k, p in tr.named_parameters()}
    got["x"], got["cond"] = x.grad, cond.grad
    _judge(case, got)


# ----------------------------------------------------------------------------- the model
def _model(case):
    import voicebox_pytorch_amd as vbx

    t = bc.inputs(case)
    vb = vbx.VoiceBox(dim=case.dim, num_cond_tokens=500, depth=2, dim_head=bc.DIM_HEAD, heads=bc.HEADS, condition_on_text=False)
    missing = vb.load_state_dict(t["state"], strict=False)
    assert not missing.unexpected_keys and all("inv_freq" in k for k in missing.missing_keys)
    vb = vb.to(dev)
    return t, vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def _draws(t):
    from voicebox_pytorch_amd.masks import rng_override

    return rng_override(x0=t["x0"], times=t["times"], frac_lengths=t["frac"], rand=t["rand"])


def _check_loss(case, loss):
    got, want = float(loss.detach()), bc.loss32_emulated(case)
    print(f"[block] {case.name}: loss {got:.6f}, emulated fp32 oracle {want:.6f}")
    assert abs(got - want) < bc.LOSS_ABS, (got, want)


MODEL_SHAPES = [(512, 3, 189, True), (1024, 3, 189, True), (512, *FULL, False), (1024, *FULL, False)]


@pytest.mark.parametrize("dim,B,N,masked", MODEL_SHAPES)
def test_model_block_grads(dim, B, N, masked):
    """wrapper(x1, mask=).backward(): every parameter's gradient materialised"""
    case = bc.Case("model", dim, B, N, masked)
    t, vb, wrapper = _model(case)
    with _draws(t):
        loss = wrapper(t["x1"].to(dev), mask=t["mask"].to(dev) if masked else None)
    loss.backward()
    _check_loss(case, loss)
    got = {k: p.grad for k, p in vb.named_parameters() if p.grad is not None}
    _judge(case, got)


@pytest.mark.parametrize("dim,B,N,masked", [(512, 3, 189, True), (512, *FULL, False), (1024, *FULL, False)])
def test_factor_form_block_grads(dim, B, N, masked):
    """The call TrainStep.step makes: _forward_backward(..., on_stage=None, adaln_factors=True) -- the adaLN weight gradients stay in
    factor form (dada_l^T . temb is layer l's (g1, b1, g2, b2) weight block), the slab reduce of all layers is deferred to one
    launch, every other gradient lands in the flat buffer."""
    from voicebox_pytorch_amd.dp import TrainStep

    case = bc.Case("model", dim, B, N, masked)
    t, vb, wrapper = _model(case)
    step = TrainStep(wrapper)
    assert step.adaln_factors_apply(batch=B)
    with _draws(t):
        loss = step._forward_backward(t["x1"].to(dev), t["mask"].to(dev) if masked else None, None, on_stage=None, adaln_factors=True)
    _check_loss(case, loss)
    eng, fp = step._last_eng, step.fp
    names = {id(p): k for k, p in vb.named_parameters()}
    got = {names[id(fp.slots[s])]: g for s, g in zip(fp.order, fp.grad_views(step.gflat)) if id(fp.slots[s]) in names}
    dada, temb = eng.adaln_factor_tensors()
    assert tuple(dada.shape) == (2, B, 4 * dim) and tuple(temb.shape) == (B, 4 * dim)
    r = _reference(case)
    ref = dict(r.grads)
    for l in range(2):
        keys = [f"transformer.layers.{l}.{n}.weight" for n in ("2.to_gamma", "2.to_beta", "4.to_gamma", "4.to_beta")]
        for k in keys:
            del got[k]  # the factor form leaves these blocks of the flat buffer unwritten
        got[f"transformer.layers.{l}.adaln_w"] = dada[l].double().t() @ temb.double()
        ref[f"transformer.layers.{l}.adaln_w"] = torch.cat([ref.pop(k) for k in keys], dim=0)
    label = case.name + "-factors"
    errs = bc.errors({k: v.detach().cpu() for k, v in got.items()}, ref)
    for line in bc.report(label, errs, r.s_case, r.S_case):
        print("[block] " + line)
    bc.check(label, errs, r.s_case, r.S_case, verbose=False)


# ----------------------------------------------------------------------------- the full-route shape gets the benchmark's kernels
def _layer_descs(L, dim, B, N):
    """The descriptors runtime.hip builds for the GEMMs of one layer, forward and backward (tests/native/gemm_route_check.cpp has the
    same table in C++), with placeholder buffers: vbx_gemm_route tests pointers for null and alignment only."""
    inner, Fp, Np = bc.HEADS * bc.DIM_HEAD, (dim * 4 * 2 // 3 + 63) // 64 * 64, N + bc.REGISTERS
    M, p = B * Np, 4096

    def desc(mode, epi, m, n, k, **kw):
        d = L.GemmDesc()
        d.mode, d.epilogue, d.M, d.N, d.K = mode, epi, m, n, k
        d.A = d.B = d.C = p
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    nt_f32 = lambda m, n, k: desc(L.VBX_GEMM_NT, L.VBX_EPI_F32, m, n, k, lda=k, ldb=k, ldc=n, f16=1)
    nn = lambda m, n, k: desc(L.VBX_GEMM_NN, L.VBX_EPI_BF16, m, n, k, lda=k, ldb=n, ldc=n)
    tn = lambda i, j, k: desc(L.VBX_GEMM_TN, L.VBX_EPI_SPLITK, i, j, k, lda=i, ldb=j, splits=3)
    return {
        "to_qkv": desc(L.VBX_GEMM_NT, L.VBX_EPI_QKV, M, 3 * inner, dim, lda=dim, ldb=dim, f16=1, Np=Np, H=bc.HEADS, qk_scale=8.0,
                       q_gamma=p, k_gamma=p, rot_cos=p, rot_sin=p, q16=p, k16=p, v16=p, qb=p, kb=p, v=p, q_rnorm=p, k_rnorm=p),
        "to_out": nt_f32(M, dim, inner),
        "ff_in": desc(L.VBX_GEMM_NT, L.VBX_EPI_GEGLU, M, 2 * Fp, dim, lda=dim, ldb=dim, ldc=Fp, f16=1, bias=p, C2=p, C3=p),
        "ff_out": nt_f32(M, dim, Fp),
        "dgrad ff_out": nn(M, Fp, dim),
        "dgrad ff_in": nn(M, dim, 2 * Fp),
        "dgrad to_out": nn(M, inner, dim),
        "dgrad to_qkv": nn(M, dim, 3 * inner),
        "wgrad to_qkv": tn(3 * inner, dim, M),
        "wgrad to_out": tn(dim, inner, M),
        "wgrad ff_in": tn(2 * Fp, dim, M),
        "wgrad ff_out": tn(dim, Fp, M),
    }


@pytest.mark.parametrize("dim", [512, 1024])
def test_full_route_shape_gets_the_benchmarks_kernels(dim):
    from voicebox_pytorch_amd import _lib as L

    L.lib()
    L.call("vbx_check_device", 0)
    here, bench = _layer_descs(L, dim, *FULL), _layer_descs(L, dim, *BENCH)
    routes = {}
    for name in here:
        a, b = L.lib().vbx_gemm_route(here[name]), L.lib().vbx_gemm_route(bench[name])
        assert a > 0 and b > 0, (name, a, b, L.lib().vbx_last_error().decode())
        routes[name] = (a, b)
    print(f"[block] dim {dim}: vbx_gemm_route at {FULL[0]} x {FULL[1] + bc.REGISTERS} / {BENCH[0]} x {BENCH[1] + bc.REGISTERS} rows: {routes}")
    assert all(a == b for a, b in routes.values()), routes
