"""The sampler kernels of csrc/ode.hip on their own (tests/ode_check.py has the cases, the fp32 stand-ins, the fp64 references and the
counted bounds; tests/test_ode_check_cpu.py shows on the CPU that the stand-in passes them and planted faults do not): vbx_ode_combine /
_dp by bits against the unfused fp32 sum and per element against fp64, vbx_ode_stage_time / _dp by bits, vbx_ode_norm / _lens (slab
sums at (n + 2) 2^-53 over the kept elements, every slot of the step state, every branch of the controller, the initial step against ode_ref),
vbx_ode_commit, vbx_ode_dense, vbx_zero_tail_rows, and the copies a forward starts with -- vbx_pack_embed_input, vbx_stack_input,
vbx_unet_cat / _split / _addskip, vbx_copy_cols_f32 -- by bits, at the sizes where the grid-stride loops and the controller's slab loop
take a second trip.

Every output buffer starts as NaN sentinels with a guard behind it, every operand element a launch must not read is NaN, every state
slot a launch must not write holds a sentinel of its own.  Each case is a launch or two, a synchronize, and ode_check's checks on CPU
copies.

Several cases write 16 MiB through a grid-stride loop's second trip, where a wrong index is an access out of bounds.  Every copy to
and from the device and every synchronize therefore goes through on_device(): an error the device reports there ends the session,
so that the cases behind it launch nothing on a device that has faulted (the other *_edges_gpu.py files stay as they are)."""
import ctypes as C

import pytest
import torch

import ode_check as oc

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


def on_device(fn):
    try:
        return fn()
    except RuntimeError as e:  # torch reports a fault of an earlier launch at its next call
        pytest.exit(f"the device reported an error after a launch of these tests, nothing more is launched: {e}", returncode=3)


def up(t):
    return None if t is None else on_device(lambda: t.contiguous().to(dev))


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def floats(vals):
    return None if vals is None else (C.c_float * len(vals))(*vals)


def cpu(**d):
    on_device(torch.cuda.synchronize)
    return {k: None if t is None else on_device(t.cpu) for k, t in d.items()}


def _ids(c):
    return getattr(c, "name", None) or "-".join(map(str, c))


# ------------------------------------------------------------------------------------------------ A. combine
@pytest.mark.parametrize("c", oc.COMBINE_CASES, ids=_ids)
def test_combine(L, c):
    ops = oc.combine_operands(c)
    y, k = up(ops["y"]), [up(t) for t in ops["k"]]
    out = y if c.inplace else up(ops["out"])
    if c.form == "table":
        L.call("vbx_ode_combine", out, y, ptrs(k), c.S, up(ops["table"]), c.ld, up(ops["counter"]), c.stride, c.row, c.n, st())
    else:
        L.call("vbx_ode_combine_dp", out, y, ptrs(k), floats(ops["beta"]), c.S, up(ops["state"]), oc.DP_DT if c.form == "dt" else oc.DP_H0, c.n, st())
    oc.check_combine(c, cpu(out=out, y=y))


# ------------------------------------------------------------------------------------------------ B. stage times
@pytest.mark.parametrize("c", oc.TIME_CASES, ids=_ids)
def test_stage_time(L, c):
    ops = oc.time_operands(c)
    times = up(ops["times"])
    if c.mode == "table":
        L.call("vbx_ode_stage_time", times, c.B, up(ops["table"]), up(ops["counter"]), ops["stride"], ops["slot"], st())
    else:
        L.call("vbx_ode_stage_time_dp", times, c.B, up(ops["state"]), ops["alpha"], ops["tmode"], st())
    oc.check_time(c, cpu(times=times))


# ------------------------------------------------------------------------------------------------ C. the norms and the controller
@pytest.mark.parametrize("c", oc.NORM_CASES, ids=_ids)
def test_norm(L, c):
    ops = oc.norm_operands(c)
    assert L.lib().vbx_ode_norm_slab_doubles(c.n) == 2 * c.nb
    state, slab, k = up(ops["state"]), up(ops["slab"]), [up(t) for t in ops["k"]]
    args = (state, slab, c.mode, up(ops["y0"]), up(ops["y1"]), ptrs(k), floats(ops["coef"]), c.S, c.n, c.nfe)
    if c.shape is None:
        L.call("vbx_ode_norm", *args, st())
    else:
        L.call("vbx_ode_norm_lens", *args, up(ops["lens"]), c.shape[0], c.shape[2], st())
    oc.check_norm(c, cpu(state=state, slab=slab))


def test_powf_sweep(L):
    """powf of the initial step read back through vbx_ode_norm (INIT1) over ode_check.POW_SWEEP against fp64: the figure the bound's
    term RHO_POW was made from still holds."""
    ms = oc.pow_sweep_values()
    rows = [oc.pow_sweep_operands(m) for m in ms]
    state, slab, y0 = (up(torch.stack([r[k] for r in rows])) for k in ("state", "slab", "y0"))
    f0, f1 = (up(torch.stack([r["k"][j] for r in rows])) for j in (0, 1))
    for i in range(len(rows)):
        L.call("vbx_ode_norm", state[i], slab[i], oc.NORM_INIT1, y0[i], None, ptrs([f0[i], f1[i]]), None, 2, 4, 1, st())
    got = cpu(state=state, slab=slab)
    ck = oc.OdeChecks("powf-sweep")
    errs = [oc.pow_sweep_error(m, s[oc.DP_DT]) for m, s in zip(ms, got["state"])]
    worst = max(range(len(errs)), key=lambda i: errs[i] if errs[i] == errs[i] else oc.INF)
    ck.le(f"largest relative error of DT = powf(0.01f / m, 0.2f) over m = 2^-24 ... 2^24, at m = {float(ms[worst]):.6g}", errs[worst], oc.POWF_REL_MEASURED)
    want = torch.stack([r["state"] for r in rows])
    want[:, oc.DP_DT], want[:, oc.DP_NFE] = got["state"][:, oc.DP_DT], 1.0
    ck.same_bits("every other slot, the guards included", got["state"], want)
    ck.true("the slabs hold (2^20 m)^2 x 4 and 0", bool((got["slab"][:, 0] == 4 * (ms.double() * 2.0 ** 20) ** 2).all()) and bool((got["slab"][:, 1] == 0).all()))
    ck.done()


# ------------------------------------------------------------------------------------------------ D, E. commit, dense output
@pytest.mark.parametrize("c", oc.COMMIT_CASES, ids=_ids)
def test_commit(L, c):
    ops = {k: up(v) for k, v in oc.commit_operands(c).items()}
    L.call("vbx_ode_commit", ops["y"], ops["k1"], ops["y1"], ops["k7"], ops["state"], c.n, st())
    oc.check_commit(c, cpu(**ops))


@pytest.mark.parametrize("c", oc.DENSE_CASES, ids=_ids)
def test_dense(L, c):
    ops = oc.dense_operands(c)
    out, k = up(ops["out"]), [up(t) for t in ops["k"]]
    L.call("vbx_ode_dense", out, up(ops["y0"]), up(ops["y1"]), ptrs(k), floats(ops["mid"]), up(ops["state"]), c.n, st())
    oc.check_dense(c, cpu(out=out))


# ------------------------------------------------------------------------------------------------ F. zeroing the padding frames
@pytest.mark.parametrize("c", oc.ZERO_TAIL_CASES, ids=_ids)
def test_zero_tail_rows(L, c):
    ops = oc.zero_tail_operands(c)
    x = up(ops["x"])
    L.call("vbx_zero_tail_rows", x, up(ops["lens"]), c.B, c.N, c.D, st())
    oc.check_zero_tail(c, cpu(x=x))


# ------------------------------------------------------------------------------------------------ G. copies and packs
@pytest.mark.parametrize("c", oc.PACK_CASES, ids=_ids)
def test_pack_embed_input(L, c):
    ops = {k: up(v) for k, v in oc.pack_operands(c).items()}
    L.call("vbx_pack_embed_input", ops["x"], ops["cond"], ops["mask"], ops["f16"], ops["bf16"], c.B, c.N, c.D, st())
    oc.check_pack(c, cpu(f16=ops["f16"], bf16=ops["bf16"]))


@pytest.mark.parametrize("c", oc.STACK_CASES, ids=_ids)
def test_stack_input(L, c):
    ops = {k: up(v) for k, v in oc.stack_operands(c).items()}
    L.call("vbx_stack_input", ops["x"], ops["reg"], ops["xs"], c.B, c.N, c.R, c.D, st())
    oc.check_stack(c, cpu(xs=ops["xs"]))


@pytest.mark.parametrize("c", oc.UNET_CASES, ids=_ids)
def test_unet_glue(L, c):
    ops = {k: up(v) for k, v in oc.unet_operands(c).items()}
    if c.kind == "cat":
        L.call("vbx_unet_cat", ops["x"], ops["skip"], c.scale, ops["f16"], ops["bf16"], c.rows, c.D, st())
        oc.check_unet(c, cpu(f16=ops["f16"], bf16=ops["bf16"]))
        return
    if c.kind == "split":
        L.call("vbx_unet_split", ops["dcat"], c.scale, ops["dx"], ops["bf16"], ops["dskip"], c.rows, c.D, st())
    else:
        L.call("vbx_unet_addskip", ops["dx"], ops["bf16"], ops["dskip"], c.rows * c.D, st())
    oc.check_unet(c, cpu(dx=ops["dx"], bf16=ops["bf16"], dskip=ops["dskip"]))


@pytest.mark.parametrize("c", oc.COPY_COLS_CASES, ids=_ids)
def test_copy_cols(L, c):
    rows, cols, ld = c
    dst = up(oc.out_buf(rows * cols))
    L.call("vbx_copy_cols_f32", up(oc.with_guard(oc.copy_cols_input(c))), ld, dst, rows, cols, st())
    oc.check_copy_cols(c, cpu(dst=dst))
