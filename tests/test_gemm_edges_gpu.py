"""Every GEMM kernel behind vbx_gemm at its own tile edges, per element against fp64 (tests/gemm_check.py has the cases, the references
and the bounds; tests/test_gemm_check_cpu.py shows on the CPU that a correct result passes them and planted faults do not).

Each case first asserts that vbx_gemm_route answers the kernel the case is meant for under its select -- a routing change that moves a
shape to another kernel fails here instead of silently removing coverage -- and then launches once dense and once with strided lda /
ldb / ldc, NaN in every operand element outside the logical extent and a sentinel around every output."""
import ctypes

import pytest
import torch

import gemm_check as gc
from gemm_check import CASES, GROUPED_JOBS

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    assert (gc.NT, gc.NN, gc.TN) == (_lib.VBX_GEMM_NT, _lib.VBX_GEMM_NN, _lib.VBX_GEMM_TN)
    assert (gc.EPI_BF16, gc.EPI_F32, gc.EPI_QKV, gc.EPI_GEGLU, gc.EPI_SPLITK, gc.EPI_GELU) == (
        _lib.VBX_EPI_BF16, _lib.VBX_EPI_F32, _lib.VBX_EPI_QKV, _lib.VBX_EPI_GEGLU, _lib.VBX_EPI_SPLITK, _lib.VBX_EPI_GELU)
    assert gc.GEMM5 == _lib.VBX_GEMM_KERNEL_GEMM5
    yield _lib
    _lib.lib().vbx_gemm_select(0)
    _lib.lib().vbx_gemm5_cu_limit(0)


def st():
    return torch.cuda.current_stream().cuda_stream


def _desc(L, built):
    """(vbx_gemm_desc, device inputs, device outputs) of a built case."""
    ins = {n: b.to(dev) for n, (b, _) in built.inputs.items()}
    outs = {n: spec.new().to(dev) for n, spec in built.outs.items()}
    d = L.GemmDesc()
    for k, v in built.scal.items():
        setattr(d, k, v)
    for field, (where, n) in built.ptrs.items():
        if where == "in":
            t, off = ins[n], built.inputs[n][1]
            setattr(d, field, t.data_ptr() + off * t.element_size())
        else:
            setattr(d, field, outs[n].data_ptr())
    return d, ins, outs


def _reduce(L, built, outs):
    c, dst = built.case, built.outs["sum"]
    L.call("vbx_splitk_reduce", outs["slabs"], c.splits, c.M, c.N, outs["sum"], c.M, c.N, dst.ld, 0, 0, 0, st())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gemm_edges(L, case):
    built = gc.build(case)
    d, ins, outs = _desc(L, built)
    lib = L.lib()
    try:
        assert lib.vbx_gemm_select(case.select) == 0
        if case.cu_limit:
            assert lib.vbx_gemm5_cu_limit(case.panels + case.cu_limit - 1) == 0
        route = lib.vbx_gemm_route(d)
        assert route == case.kernel, f"{case.name}: routed to {route}, meant for {case.kernel}: {lib.vbx_last_error().decode()}"
        rc = lib.vbx_gemm(d, st())
        assert rc == 0, lib.vbx_last_error().decode()
    finally:
        lib.vbx_gemm5_cu_limit(0)
        lib.vbx_gemm_select(0)
    if case.epi == gc.EPI_SPLITK:
        _reduce(L, built, outs)
    torch.cuda.synchronize()
    gc.check(built, {n: t.cpu() for n, t in outs.items()})


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_grouped_splitk_edges(L, n, strided):
    """vbx_gemm_tn_splitk_grouped with 1 .. 4 jobs in one launch of the 256 x 256 tile: odd K, K = 40, M = N = 8, an empty split."""
    jobs = [gc.build(gc.replace(c, strided=strided)) for c in GROUPED_JOBS[:n]]
    descs = (L.GemmDesc * n)()
    keep = []
    for i, b in enumerate(jobs):
        d, ins, outs = _desc(L, b)
        ctypes.memmove(ctypes.addressof(descs[i]), ctypes.addressof(d), ctypes.sizeof(d))
        keep.append((ins, outs))
    lib = L.lib()
    assert lib.vbx_gemm_select(0) == 0
    rc = lib.vbx_gemm_tn_splitk_grouped(descs, n, st())
    assert rc == 0, lib.vbx_last_error().decode()
    for b, (_, outs) in zip(jobs, keep):
        _reduce(L, b, outs)
    torch.cuda.synchronize()
    for b, (_, outs) in zip(jobs, keep):
        gc.check(b, {k: t.cpu() for k, t in outs.items()}, label=f"grouped{n}-{b.case.name}")


# ----------------------------------------------------------------------------- argument checks
def _valid(L, mode, epi, M=64, N=64, K=64):
    d = L.GemmDesc()
    d.mode, d.epilogue, d.M, d.N, d.K, d.splits = mode, epi, M, N, K, 1
    d.lda = M if mode == gc.TN else K
    d.ldb = K if mode == gc.NT else N
    d.ldc = N
    d.A = d.B = d.C = 4096  # vbx_gemm_route only tests pointers for null and alignment; an invalid descriptor is refused before any use
    return d


BAD_ARGS = [
    ("nt-lda<K", gc.NT, gc.EPI_BF16, dict(lda=56)),
    ("nn-lda<K", gc.NN, gc.EPI_F32, dict(lda=56)),
    ("tn-lda<M", gc.TN, gc.EPI_SPLITK, dict(lda=56)),
    ("nt-ldb<K", gc.NT, gc.EPI_F32, dict(ldb=56)),
    ("nn-ldb<N", gc.NN, gc.EPI_BF16, dict(ldb=56)),
    ("tn-ldb<N", gc.TN, gc.EPI_SPLITK, dict(ldb=56)),
    ("bf16-ldc<N", gc.NT, gc.EPI_BF16, dict(ldc=56)),
    ("f32-ldc<N", gc.NN, gc.EPI_F32, dict(ldc=56)),
    ("bf16-ldc=0", gc.NT, gc.EPI_BF16, dict(ldc=0)),
    # the k-contiguous A of NN is staged in 16-byte pieces like NT's operands: a ragged K would read the row padding (include/vbx.h)
    ("nn-K%8", gc.NN, gc.EPI_F32, dict(K=60)),
    ("nn-K%8-bf16", gc.NN, gc.EPI_BF16, dict(K=63)),
    ("nt-K%8", gc.NT, gc.EPI_BF16, dict(K=60)),
]


@pytest.mark.parametrize("name,mode,epi,bad", BAD_ARGS, ids=[b[0] for b in BAD_ARGS])
@pytest.mark.parametrize("select", [0, 1, 2, 3])
def test_bad_leading_dimensions_are_refused(L, select, name, mode, epi, bad):
    """vbx_gemm and vbx_gemm_route answer VBX_EINVAL, whichever kernel is selected, and launch nothing."""
    lib = L.lib()
    good = _valid(L, mode, epi)
    d = _valid(L, mode, epi)
    for k, v in bad.items():
        setattr(d, k, v)
    try:
        assert lib.vbx_gemm_select(select) == 0
        assert lib.vbx_gemm_route(good) > 0, lib.vbx_last_error().decode()  # the same descriptor without the fault is served
        assert lib.vbx_gemm_route(d) == -1 and lib.vbx_gemm(d, st()) == -1  # VBX_EINVAL
    finally:
        lib.vbx_gemm_select(0)
    torch.cuda.synchronize()


def test_tn_takes_any_k(L):
    """TN stages both operands k-strided, one k row per piece: odd K stays valid (and is launched by the split-K cases above)."""
    d = _valid(L, gc.TN, gc.EPI_SPLITK, K=63)
    assert L.lib().vbx_gemm_route(d) == gc.BM128
