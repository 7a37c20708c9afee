"""The aligner primitives on the device (csrc/align.hip) against tests/align_ref.py in fp64: maximum_path bit-equal on integer scores
(ties included), valid and within the derived bound of the optimum on Gaussian scores; forward_sum_loss / ForwardSumLoss within
4 x the error of torch's own fp32 CPU construction on the same inputs (value and gradient), zeros outside the lengths; reruns,
batch independence, input layouts.  Parity with naturalspeech2_pytorch is UNPINNED (the library is absent).

Measured (MI355X, `pytest -s -m gpu tests/test_align_gpu.py` prints the lines kept in profiles/align_parity.txt)."""
import pytest
import torch

import align_ref as ar

gpu = pytest.mark.gpu
dev = "cuda"

CASES = [(B, T, K, i) for B, T, K in ar.SHAPES for i in range(len(ar.length_batches(B, T, K)))]
IDS = [f"{B}x{T}x{K}-lens{i}" for B, T, K, i in CASES]


@pytest.fixture(scope="module")
def vbx():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return vbx


def lens_dev(lens):
    return torch.tensor(lens, dtype=torch.int64, device=dev)


# ----------------------------------------------------------------------------- maximum_path
@gpu
@pytest.mark.parametrize("B,T,K,batch", CASES, ids=IDS)
def test_maximum_path_integer_scores_bit_equal(vbx, B, T, K, batch):
    """integers in [-3, 3]: every fp32 sum is exact, so path and durations equal the fp64 restatement bit for bit, ties included"""
    value, qlens, klens, want, want_dur, _, _ = ar.path_reference("int", B, T, K, batch)
    path, dur = vbx.maximum_path(value.to(dev), lens_dev(qlens), lens_dev(klens))
    assert path.shape == value.shape and path.dtype == torch.float32 and dur.dtype == torch.int64 and dur.shape == (B, K)
    assert not path.requires_grad
    path, dur = path.cpu(), dur.cpu()
    assert torch.equal(path.double(), want), [int((path[b].double() != want[b]).sum()) for b in range(B)]
    assert torch.equal(dur, want_dur)
    for b in range(B):
        if qlens[b] < klens[b]:
            assert not bool(path[b].any()) and not bool(dur[b].any())


@gpu
@pytest.mark.parametrize("B,T,K,batch", CASES, ids=IDS)
def test_maximum_path_gaussian_scores_valid_and_within_the_bound(vbx, B, T, K, batch):
    value, qlens, klens, _, _, best, qmax = ar.path_reference("gauss", B, T, K, batch)
    path, dur = vbx.maximum_path(value.to(dev), lens_dev(qlens), lens_dev(klens))
    path, dur = path.cpu(), dur.cpu()
    assert ar.path_problems(path, dur, qlens, klens) == []
    score = ar.path_score(path, value)
    for b in range(B):
        if best[b] is None:
            continue
        bound = ar.path_bound(T, qmax[b])
        gap = best[b] - float(score[b])
        print(f"maximum_path {B}x{T}x{K} lens {qlens[b]}/{klens[b]}: optimum {best[b]:.6f} gap {gap:.3e} bound {bound:.3e}")
        assert -1e-9 * max(1.0, abs(best[b])) <= gap <= bound, (b, gap, bound)


# ----------------------------------------------------------------------------- forward-sum
@gpu
@pytest.mark.parametrize("B,T,K,batch", CASES, ids=IDS)
def test_forward_sum_against_fp64_within_four_times_the_fp32_cpu_error(vbx, B, T, K, batch):
    ref = ar.loss_reference(B, T, K, batch)
    tol = ar.loss_tolerances(ref, T)
    qlens, klens = ref["qlens"], ref["klens"]
    kl, ql = lens_dev(klens), lens_dev(qlens)

    x = ref["x"].to(dev).requires_grad_(True)
    nll = vbx.forward_sum_loss(x, kl, ql, reduction="none")
    assert nll.shape == (B,) and nll.dtype == torch.float32
    g_sum, = torch.autograd.grad(nll.sum(), x)
    x2 = ref["x"].to(dev).requires_grad_(True)
    mean = vbx.forward_sum_loss(x2, kl, ql)
    g_mean, = torch.autograd.grad(mean, x2)
    x3 = ref["x"].to(dev).requires_grad_(True)
    module_mean = vbx.ForwardSumLoss(blank_logprob=-1.)(x3, kl, ql)
    g_module, = torch.autograd.grad(module_mean, x3)
    assert torch.equal(module_mean, mean) and torch.equal(g_module, g_mean)
    assert g_sum.shape == x.shape and g_sum.dtype == torch.float32

    err = dict(nll=(nll.detach().cpu().double() - ref["nll"]).abs(), mean=abs(float(mean.detach()) - float(ref["mean"])),
               g_sum=float((g_sum.cpu().double() - ref["g_sum"]).abs().max()),
               g_mean=float((g_mean.cpu().double() - ref["g_mean"]).abs().max()))
    cpu = ref["cpu_err"]
    print(f"forward_sum {B}x{T}x{K} lens q{qlens} k{klens}: |nll| max {float(ref['nll'].abs().max()):.3f}; "
          f"nll err kernel {float(err['nll'].max()):.3e} fp32-CPU {float(cpu['nll'].max()):.3e} allowed {float(tol['nll'].max()):.3e}; "
          f"mean err kernel {err['mean']:.3e} fp32-CPU {cpu['mean']:.3e} allowed {tol['mean']:.3e}; "
          f"grad(sum nll) err kernel {err['g_sum']:.3e} fp32-CPU {cpu['g_sum']:.3e} allowed {tol['g_sum']:.3e} "
          f"(max |grad| {float(ref['g_sum'].abs().max()):.3e}); "
          f"grad(mean) err kernel {err['g_mean']:.3e} fp32-CPU {cpu['g_mean']:.3e} allowed {tol['g_mean']:.3e}")
    # exact zeros: outside the lengths and on the row without a path
    for g in (g_sum.cpu(), g_mean.cpu()):
        for b in range(B):
            q, k = qlens[b], klens[b]
            if q < k:
                assert not bool(g[b].any())
            else:
                assert not bool(g[b, q:].any()) and not bool(g[b, :, k:].any())
    for b in range(B):
        if qlens[b] < klens[b]:
            assert float(nll[b].detach()) == 0.0
    assert bool((err["nll"] <= tol["nll"]).all()), (err["nll"], tol["nll"])
    assert err["mean"] <= tol["mean"], (err["mean"], tol["mean"])
    assert err["g_sum"] <= tol["g_sum"], (err["g_sum"], tol["g_sum"])
    assert err["g_mean"] <= tol["g_mean"], (err["g_mean"], tol["g_mean"])


# ----------------------------------------------------------------------------- both ops
SMALL = [(3, 70, 65, 0), (2, 200, 129, 1), (3, 129, 9, 0)]


def run_both(vbx, value, x, qlens, klens):
    ql, kl = lens_dev(qlens), lens_dev(klens)
    path, dur = vbx.maximum_path(value, ql, kl)
    xg = x.detach().clone().requires_grad_(True)
    nll = vbx.forward_sum_loss(xg, kl, ql, reduction="none")
    grad, = torch.autograd.grad(nll.sum(), xg)
    return path, dur, nll.detach(), grad


@gpu
@pytest.mark.parametrize("B,T,K,batch", SMALL, ids=[f"{B}x{T}x{K}" for B, T, K, _ in SMALL])
def test_reruns_rows_alone_layouts_and_strides_agree_bitwise(vbx, B, T, K, batch):
    qlens, klens = ar.length_batches(B, T, K)[batch]
    value, x = ar.gaussian_scores(B, T, K).to(dev), ar.loss_inputs(B, T, K).to(dev)
    first = run_both(vbx, value, x, qlens, klens)
    again = run_both(vbx, value, x, qlens, klens)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for i in range(B):  # a row alone is the same row inside the batch
        alone = run_both(vbx, value[i:i + 1], x[i:i + 1], qlens[i:i + 1], klens[i:i + 1])
        assert all(torch.equal(a[0], b[i]) for a, b in zip(alone, first)), i
    four = run_both(vbx, value[:, None], x[:, None], qlens, klens)  # [B, 1, T, K]
    assert four[0].shape == (B, 1, T, K) and four[3].shape == (B, 1, T, K)
    assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(four, first))
    # non-contiguous: the same values as a transposed view of a [B, K, T] buffer
    strided = run_both(vbx, value.transpose(1, 2).contiguous().transpose(1, 2), x.transpose(1, 2).contiguous().transpose(1, 2), qlens, klens)
    assert not x.transpose(1, 2).contiguous().transpose(1, 2).is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(strided, first))


@gpu
def test_default_lengths_other_dtypes_and_no_grad(vbx):
    B, T, K = 2, 40, 17
    value, x = ar.gaussian_scores(B, T, K).to(dev), ar.loss_inputs(B, T, K).to(dev)
    full = run_both(vbx, value, x, [T] * B, [K] * B)
    path, dur = vbx.maximum_path(value)
    assert torch.equal(path, full[0]) and torch.equal(dur, full[1])
    assert torch.equal(vbx.forward_sum_loss(x, reduction="none"), full[2])
    assert torch.equal(vbx.forward_sum_loss(x), (full[2] / K).mean())
    int32 = vbx.maximum_path(value, torch.tensor([T, T], dtype=torch.int32, device=dev), None)[0]
    assert torch.equal(int32, path)
    half = value.to(torch.bfloat16)
    p16, d16 = vbx.maximum_path(half)
    assert p16.dtype == torch.bfloat16
    p32, d32 = vbx.maximum_path(half.float())
    assert torch.equal(p16.float(), p32) and torch.equal(d16, d32)
    with torch.no_grad():
        assert torch.equal(vbx.forward_sum_loss(x, reduction="none"), full[2])
    # a different blank changes the loss the way the restatement says
    got = vbx.forward_sum_loss(x, blank_logprob=-3.0, reduction="none").cpu().double()
    want = ar.forward_sum_ref(x.cpu().double(), [K] * B, [T] * B, -3.0, "none")
    cpu = ar.ctc_construction(x.cpu(), [K] * B, [T] * B, -3.0, "none").double()
    allowed = torch.maximum(4.0 * (cpu - want).abs(), T * 2.0 ** -23 * want.abs().clamp(min=1.0))
    assert bool(((got - want).abs() <= allowed).all()) and float((want - full[2].cpu().double()).abs().min()) > 1.0
    with pytest.raises(ValueError, match="device"):
        vbx.maximum_path(value, torch.tensor([T, T]), None)
