"""The conditioning and loss kernels of csrc/ops.hip on their own, per element against fp64 (tests/ops_check.py has the cases, the
references and the counted bounds; tests/test_ops_check_cpu.py shows on the CPU that the fp32 stand-in passes them and planted faults do
not): vbx_time_embed_fwd / _bwd, vbx_adaln_proj_fwd on both of its kernels, vbx_adaln_proj_bwd on both of its kernels,
vbx_adaln_dtemb_all with the wide row sum, vbx_sum_rows_f32, vbx_geglu_bwd / _colsum, vbx_colsum_bf16 / _partials / _f32,
vbx_multi_reduce, vbx_masked_mse_fwd / _bwd, vbx_cfm_inputs, vbx_axpy_dev / _ctr, vbx_ada_select and vbx_counter_add, at the shapes
where their guards, dispatches, slice seams and grid caps decide.

Every output buffer starts as NaN sentinels with a guard row behind it, every operand row a launch must not read is NaN.  Each case is
a few launches, a synchronize, and ops_check's checks on CPU copies.  The case ids name the kernel a dispatch must pick (mfma / scalar,
v2 / v1); the checks assert it from the shape."""
import ctypes as C

import pytest
import torch

import ops_check as oc
from rows_check import nan_guard

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def up(t):
    return None if t is None else t.contiguous().to(dev)


def ups(d):
    return {k: up(t) for k, t in d.items()}


def cpu(d):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in d.items()}


# ------------------------------------------------------------------------------------------------ A. time embedding
@pytest.mark.parametrize("c", oc.TIME_CASES, ids=lambda c: c.name)
def test_time_embed(L, c):
    inp = oc.time_inputs(c)
    times, wsin, w1, b1 = up(inp["times"]), up(inp["wsin"]), up(nan_guard(inp["w1"], c.D)), up(inp["b1"])
    out = ups(oc.new_time_out(c))
    assert L.lib().vbx_time_embed_bwd_scratch_floats(c.B, c.D) == oc.time_scratch_floats(c)
    L.call("vbx_time_embed_fwd", times, wsin, w1, b1, out["four"], out["pre"], out["temb"], c.B, c.D, c.Th, st())
    L.call("vbx_time_embed_bwd", times, wsin, w1, up(nan_guard(inp["four"], c.D)), up(nan_guard(inp["pre"], c.Th)),
           up(nan_guard(inp["dtemb"], c.Th)), out["dw_sin"], out["dw1"], out["db1"], out["scratch"], c.B, c.D, c.Th, st())
    oc.check_time(c, cpu(out))


def test_time_embed_refuses_an_odd_width(L):
    z = torch.zeros(64, device=dev)
    for name, args in (("vbx_time_embed_fwd", (z, z, z, z, z, z, z, 1, 3, 1, st())), ("vbx_time_embed_bwd", (z, z, z, z, z, z, z, z, z, z, 1, 3, 1, st()))):
        with pytest.raises(L.VbxError, match="bad args"):
            L.call(name, *args)


def test_time_libm_sweep(L):
    """sinf / cosf and the SiLU's expf read back through vbx_time_embed_fwd over the sweeps of ops_check against fp64: the figures the
    bounds' terms A_SINCOS and RHO_SILU were made from still hold."""
    sw = oc.time_sweep_inputs()
    D, Th = sw["D"], sw["Th"]
    four, pre, temb = (up(oc.rows_buf(1, n, oc.F32)) for n in (D, Th, Th))
    L.call("vbx_time_embed_fwd", up(sw["times"]), up(sw["wsin"]), torch.zeros(Th, D, device=dev), up(sw["b1"]), four, pre, temb, 1, D, Th, st())
    torch.cuda.synchronize()
    four, pre, temb = four.cpu(), pre.cpu(), temb.cpu()
    e_sc, e_silu = oc.time_sweep_errors(sw, four[:1], pre[:1], temb[:1])
    ck = oc.OpsChecks("time-libm-sweep")
    ck.le("largest |four - sin / cos(f)| over |f| <= 32", e_sc, oc.SINCOS_ABS_MEASURED)
    ck.le("largest relative error of temb against the fp64 SiLU over |pre| <= 8", e_silu, oc.SILU_REL_MEASURED)
    ck.same_bits("pre = b1", pre[0], sw["b1"])
    ck.sentinel_kept("guard rows", torch.cat([four[1:].reshape(-1), pre[1:].reshape(-1), temb[1:].reshape(-1)]))
    ck.done()


# ------------------------------------------------------------------------------------------------ B. adaLN projection forward
def _ada_fwd(L, c):
    assert oc.fwd_kernel(c.B, c.Th) == c.kernel
    inp = oc.ada_fwd_inputs(c)
    out = ups(oc.new_ada_fwd_out(c))
    L.call("vbx_adaln_proj_fwd", up(nan_guard(inp["temb"], c.Th)), up(nan_guard(inp["w"], c.Th)), up(inp["bias"]), out["ada"], c.B, c.Th, c.J,
           c.group, st())
    oc.check_ada_fwd(c, cpu(out))


@pytest.mark.parametrize("c", [c for c in oc.ADA_FWD_CASES if c.kernel == "mfma"], ids=lambda c: c.name)
def test_adaln_fwd_mfma(L, c):
    _ada_fwd(L, c)


@pytest.mark.parametrize("c", [c for c in oc.ADA_FWD_CASES if c.kernel == "scalar" and c.Th != 4104], ids=lambda c: c.name)
def test_adaln_fwd_scalar(L, c):
    _ada_fwd(L, c)


@pytest.mark.parametrize("c", [c for c in oc.ADA_FWD_CASES if c.Th == 4104], ids=lambda c: c.name)
def test_adaln_fwd_scalar_halved_batch_chunk_dynamic_lds(L, c):
    """Th = 4104, B = 8: eight rows of temb are 131328 bytes, so bc halves to 4 and the 65664 bytes of LDS need the attribute call"""
    _ada_fwd(L, c)


# ------------------------------------------------------------------------------------------------ C. adaLN projection backward
def _ada_bwd(L, c):
    assert oc.bwd_kernel(c.J) == c.kernel
    assert L.lib().vbx_adaln_proj_bwd_scratch_floats(c.B, c.Th, c.J) == oc.ADA_SLICES * c.B * c.Th
    inp = oc.ada_bwd_inputs(c)
    out = ups(oc.new_ada_bwd_out(c))
    L.call("vbx_adaln_proj_bwd", up(nan_guard(inp["temb"], c.Th)), up(nan_guard(inp["w"], c.Th)), up(nan_guard(inp["dada"], c.J)), out.get("dw"),
           out["dbias"], out["dtemb"], out["scratch"], c.B, c.Th, c.J, c.acc, st())
    oc.check_ada_bwd(c, cpu(out))


@pytest.mark.parametrize("c", [c for c in oc.ADA_BWD_CASES if c.kernel == "v2"], ids=lambda c: c.name)
def test_adaln_bwd_v2(L, c):
    _ada_bwd(L, c)


@pytest.mark.parametrize("c", [c for c in oc.ADA_BWD_CASES if c.kernel == "v1"], ids=lambda c: c.name)
def test_adaln_bwd_v1(L, c):
    _ada_bwd(L, c)


# ------------------------------------------------------------------------------------------------ D, E. dtemb_all, the row sums
@pytest.mark.parametrize("c", oc.DTEMB_CASES, ids=lambda c: c.name)
def test_adaln_dtemb_all(L, c):
    inp = oc.dtemb_inputs(c)
    assert L.lib().vbx_adaln_dtemb_all_scratch_floats(c.L, c.B, c.Th, c.J) == c.rows * c.B * c.Th
    out = ups(oc.new_dtemb_out(c))
    L.call("vbx_adaln_dtemb_all", up(nan_guard(inp["w"], c.Th)), up(nan_guard(inp["dada"], c.J)), out["dtemb"], out["scratch"], c.L, c.B, c.Th, c.J,
           st())
    oc.check_dtemb(c, cpu(out))


@pytest.mark.parametrize("c", oc.SUM_ROWS_CASES, ids=lambda c: c.name)
def test_sum_rows(L, c):
    out = ups(oc.new_sum_rows_out(c))
    L.call("vbx_sum_rows_f32", up(oc.sum_rows_operand(c)), c.rows, c.cols + c.pad, out["out"], c.cols, c.acc, st())
    oc.check_sum_rows(c, cpu(out))


# ------------------------------------------------------------------------------------------------ F. GEGLU backward
@pytest.mark.parametrize("c", oc.GEGLU_CASES, ids=lambda c: c.name)
def test_geglu_bwd(L, c):
    inp = oc.geglu_inputs(c)
    h1, dg = up(nan_guard(inp["h1"], 2 * c.Fp)), up(nan_guard(inp["dg"], c.Fp))
    out = ups(oc.new_geglu_out(c))
    L.call("vbx_geglu_bwd", h1, dg, out["dh1"], c.M, c.Fp, st())
    if c.colsum:
        assert L.lib().vbx_geglu_bwd_colsum_slabs() == oc.GB_SLABS
        L.call("vbx_geglu_bwd_colsum", h1, dg, out["dh1_cs"], c.M, c.Fp, out["rec"], st())
    oc.check_geglu(c, cpu(out))


# ------------------------------------------------------------------------------------------------ G. column sums
@pytest.mark.parametrize("c", oc.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum(L, c):
    x = up(oc.colsum_operand(c))
    out = ups(oc.new_colsum_out(c))
    assert L.lib().vbx_colsum_slabs() == oc.CS_SLABS and L.lib().vbx_colsum_scratch_floats(c.M, c.C) == oc.CS_SLABS * c.C
    if c.kind == "bf16":
        L.call("vbx_colsum_bf16", x, c.M, c.C, c.C + c.pad, out["out"], c.n_out, c.rowmap, c.Fd, out["rec"], st())
    else:
        L.call("vbx_colsum_f32", x, c.M, c.C, c.C + c.pad, out["out"], out["rec"], st())
    oc.check_colsum(c, cpu(out))


@pytest.mark.parametrize("c", [c for c in oc.COLSUM_CASES if c.kind == "bf16" and not c.rowmap], ids=lambda c: c.name)
def test_colsum_partials(L, c):
    out = ups(oc.new_colsum_out(c))
    L.call("vbx_colsum_bf16_partials", up(oc.colsum_operand(c)), c.M, c.C, c.C + c.pad, out["rec"], st())
    oc.check_colsum(c, cpu(out), partials_only=True)


class _MrJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_bstride", C.c_long), ("dst_bstride", C.c_long), ("row_stride", C.c_long),
                ("rows", C.c_int), ("cols", C.c_int), ("batches", C.c_int), ("dst_len", C.c_int), ("rowmap", C.c_int), ("F", C.c_int),
                ("block0", C.c_int), ("pad_", C.c_int)]


class _MrJobs(C.Structure):
    _fields_ = [("job", _MrJob * oc.VBX_MR_MAX), ("n", C.c_int)]


@pytest.mark.parametrize("name", list(oc.MR_SETS), ids=str)
def test_multi_reduce(L, name):
    ks = oc.MR_SETS[name]
    src, dst = [up(oc.mr_input(k)[1]) for k in ks], [up(oc.new_mr_out(k)) for k in ks]
    jobs = _MrJobs()
    jobs.n = len(ks)
    for i, k in enumerate(ks):
        j, d = oc.MR_JOBS[k], jobs.job[i]
        d.src, d.dst, d.src_bstride, d.dst_bstride, d.row_stride = src[i].data_ptr(), dst[i].data_ptr(), j.src_bstride, j.dst_bstride, j.row_stride
        d.rows, d.cols, d.batches, d.dst_len, d.rowmap, d.F = j.rows, j.cols, j.batches, j.n_dst, j.rowmap, j.F
    lib = L.lib()
    lib.vbx_multi_reduce.argtypes = [C.POINTER(_MrJobs), C.c_void_p]
    assert lib.vbx_multi_reduce(C.byref(jobs), st()) == 0, lib.vbx_last_error()
    torch.cuda.synchronize()
    oc.check_mr(name, ks, [t.cpu() for t in dst])


# ------------------------------------------------------------------------------------------------ H. masked MSE
@pytest.mark.parametrize("c", oc.MSE_CASES, ids=lambda c: c.name)
def test_masked_mse(L, c):
    inp = oc.mse_inputs(c)
    assert L.lib().vbx_masked_mse_scratch_floats(c.B) == oc.mse_floats(c.B)
    pred, target, mask = up(nan_guard(inp["pred"], c.D)), up(nan_guard(inp["target"], c.D)), up(inp["mask"].to(torch.uint8))
    out = ups(oc.new_mse_out(c))
    L.call("vbx_masked_mse_fwd", pred, target, mask, out["per_b"], out["loss"], c.B, c.N, c.D, st())
    gs = torch.tensor([oc.GSCALE], device=dev) if c.gscale else None
    L.call("vbx_masked_mse_bwd", pred, target, mask, out["per_b"], gs, out.get("dpred"), out.get("dpb"), c.B, c.N, c.D, st())
    oc.check_mse(c, cpu(out))


# ------------------------------------------------------------------------------------------------ I. CFM inputs and the ODE glue
@pytest.mark.parametrize("c", oc.CFM_CASES, ids=lambda c: c.name)
def test_cfm_inputs(L, c):
    inp = oc.cfm_inputs(c)
    out = ups(oc.new_cfm_out(c))
    L.call("vbx_cfm_inputs", up(nan_guard(inp["x1"], c.per)), up(nan_guard(inp["x0"], c.per)), up(inp["times"]), c.sigma, out["w"], out["flow"], c.B,
           c.per, st())
    oc.check_cfm(c, cpu(out))


@pytest.mark.parametrize("n", oc.AXPY_N)
def test_axpy(L, n):
    inp = oc.axpy_inputs(n)
    y, f = up(inp["y"]), up(inp["f"])
    out = ups(oc.new_axpy_out(n))
    L.call("vbx_axpy_dev", y, f, up(inp["coef"]), oc.AXPY_IDX, out["dev"], n, st())
    L.call("vbx_axpy_ctr", y, f, up(inp["table"]), up(inp["counter"]), oc.AXPY_SLOT, out["ctr"], n, st())
    oc.check_axpy(n, cpu(out))


@pytest.mark.parametrize("c", oc.SELECT_CASES, ids=lambda c: c.name)
def test_ada_select(L, c):
    inp = oc.select_inputs(c)
    out = ups(oc.new_select_out(c))
    L.call("vbx_ada_select", out["ada"], c.L, c.B, c.G, up(inp["table"]), up(inp["counter"]), c.stride, c.slot, st())
    oc.check_select(c, cpu(out))


@pytest.mark.parametrize("inc", [1, 3, -2])
def test_counter_add(L, inc):
    t = up(oc.new_counter())
    L.call("vbx_counter_add", t[1:], inc, st())
    torch.cuda.synchronize()
    oc.check_counter(t.cpu(), inc)
