"""The optimizer kernels of the train step on their own, per element against fp64 (tests/optim_check.py has the cases, the references
and the counted bounds; tests/test_optim_check_cpu.py shows on the CPU that the fp32 stand-in passes them and planted faults do not):
vbx_adam_step_packed on synthetic segment tables, vbx_adam_adaln_factors, vbx_adaln_expand_dw, vbx_sumsq, vbx_sumsq_ranges,
vbx_sumsq_adaln_factors, vbx_clip_coef, three steps of the whole chain, and the invariants of a real model's segment table.

Every pointer is a buffer of the size the entry point may touch plus a guard row; state and destinations start as sentinels, operands
outside their extent as NaN.  Each case is one launch, a synchronize, and optim_check's checks on CPU copies."""
import ctypes as C

import pytest
import torch

import optim_check as oc
from optim_check import (CHAIN_STEPS, CLIP_CASES, EXPAND_SHAPES, FACTOR_CASES, GRAM_CASES, PACKED_CASES, RANGES_CASES, SUMSQ_CASES, TABLES)

pytestmark = pytest.mark.gpu

dev = "cuda"
HYPER = (oc.LR, oc.B1, oc.B2, oc.EPS)


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib, engine

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    engine._rt()  # the prototypes of the stage-level entry points
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def cpu(d):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in d.items()}


def _gs(gs):
    return None if gs is None else torch.tensor([gs], device=dev)


def _ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def _longs(xs):
    return (C.c_long * len(xs))(*xs)


# ----------------------------------------------------------------------------- A. vbx_adam_step_packed
def _device_table(table, dst):
    """the vbx_adam_seg table on the device, its virtual destination addresses mapped onto the buffers `dst`"""
    from voicebox_pytorch_amd.engine import VbxAdamSeg

    tab = (VbxAdamSeg * len(table.segs))()
    for row, s in zip(tab, table.segs):
        for f in oc.SEG_FIELDS:
            if f in ("dst_bf16", "dst_f16", "dst_f32"):
                setattr(row, f, _ptr(dst[table.resolve(s[f])[0]], table.resolve(s[f])[1]) if s[f] else None)
            else:
                setattr(row, f, s[f])
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)


def _adam_packed(L, table, state, g, dst, step, gs):
    raw = _device_table(table, dst)
    rc = L.lib().vbx_adam_step_packed(state["p"].data_ptr(), g.data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), raw.data_ptr(),
                                      len(table.segs), table.total_blocks, *HYPER, step, gs.data_ptr() if gs is not None else None, st())
    assert rc == 0, L.lib().vbx_last_error().decode()
    return raw


def _pack_weight_agrees(L, table, p, dst):
    """vbx_pack_weight on the device's updated p: a second, independent producer of the row-mapped layout (it also zeroes the rows the
    map pads, which the Adam launch never touches: compared where a segment maps)"""
    maps = table.dst_map()
    for i, s in enumerate(table.segs):
        if s["rowmap"] != 1 or not (s["dst_bf16"] or s["dst_f16"]):
            continue
        rows = -(-s["F"] // 64) * 128
        bname, hname = (table.resolve(s[k])[0] if s[k] else None for k in ("dst_bf16", "dst_f16"))
        fresh = {n: torch.zeros(rows * s["dst_ld"], dtype=dst[n].dtype, device=dev) for n in (bname, hname) if n}
        rc = L.lib().vbx_pack_weight(_ptr(p, s["off"]), s["count"] // s["cols"], s["cols"], _ptr(fresh[bname]) if bname else None,
                                     _ptr(fresh[hname]) if hname else None, rows, s["dst_ld"], 1, s["F"], st())
        assert rc == 0, L.lib().vbx_last_error().decode()
        torch.cuda.synchronize()
        for n, t in fresh.items():
            on = maps[n][: rows * s["dst_ld"]] >= 0
            assert bool(on.any()) and torch.equal(oc.bits(t.cpu())[on], oc.bits(dst[n].cpu())[: rows * s["dst_ld"]][on]), (table.name, i, n)


@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: c.name)
def test_adam_step_packed(L, case):
    table, inp = TABLES[case.table], oc.packed_inputs(case)
    state = {k: inp[k].to(dev) for k in "pmv"}
    dst = {n: t.to(dev) for n, t in oc.new_dst(table).items()}
    _adam_packed(L, table, state, inp["g"].to(dev), dst, case.step, _gs(case.gs))
    oc.check_packed(case, cpu({**state, **dst}))
    _pack_weight_agrees(L, table, state["p"], dst)


# ----------------------------------------------------------------------------- B. vbx_adam_adaln_factors
def _adam_factors(L, lay, state, dada, temb, fdst, B, step, gs):
    """dada, temb: (device buffer, element offset) behind a NaN front; fdst: {"f16.<l>": buffer}"""
    ptrs = (C.c_void_p * lay["L"])(*[(_ptr(fdst[f"f16.{l}"]) if f"f16.{l}" in fdst else None) for l in range(lay["L"])])
    rc = L.lib().vbx_adam_adaln_factors(state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), _longs(lay["w_off"]),
                                        ptrs if lay["dst_array"] else None, _ptr(*dada), _ptr(*temb), lay["L"], B, lay["J4"], lay["Th"],
                                        *HYPER, step, gs.data_ptr() if gs is not None else None, st())
    assert rc == 0, L.lib().vbx_last_error().decode()


def _operands(dada, temb):
    (db, do), (tb, to) = oc.embed_nan(dada), oc.embed_nan(temb)
    return (db.to(dev), do), (tb.to(dev), to)


@pytest.mark.parametrize("case", FACTOR_CASES, ids=lambda c: c.name)
def test_adam_adaln_factors(L, case):
    lay, inp = oc.factor_inputs(case)
    state = {k: inp[k].to(dev) for k in "pmv"}
    fdst = {n: t.to(dev) for n, t in oc.new_factor_dst(lay).items()}
    dada, temb = _operands(inp["dada"], inp["temb"])
    _adam_factors(L, lay, state, dada, temb, fdst, case.B, case.step, _gs(case.gs))
    oc.check_factor(case, cpu({**state, **fdst}))


# ----------------------------------------------------------------------------- C. vbx_adaln_expand_dw
@pytest.mark.parametrize("sh", EXPAND_SHAPES, ids=oc.expand_name)
def test_adaln_expand_dw(L, sh):
    B, J4, Th = sh
    dada, temb = _operands(*oc.expand_inputs(sh))
    dw = oc.new_expand_dst(sh).to(dev)
    rc = L.lib().vbx_adaln_expand_dw(_ptr(*temb), _ptr(*dada), dw.data_ptr(), B, Th, J4, 0, st())
    assert rc == 0, L.lib().vbx_last_error().decode()
    torch.cuda.synchronize()
    oc.check_expand(sh, dw.cpu())


# ----------------------------------------------------------------------------- D. the norm
def _out():
    return oc.sentinel(2, torch.float32).to(dev)  # out[0], and a guard


@pytest.mark.parametrize("n,off", SUMSQ_CASES)
def test_sumsq(L, n, off):
    x = oc.sumsq_input(n, off).to(dev)
    outs = []
    for _ in range(2):  # the second run: the same bits
        out, scratch = _out(), torch.full((1024 + 8,), float("nan"), device=dev)
        L.call("vbx_sumsq", x[off:], n, out, scratch, st())
        torch.cuda.synchronize()
        assert int(oc.bits(out.cpu())[1]) == oc.SENTINEL[torch.float32][1]
        outs.append(out.cpu()[:1])
    oc.check_sumsq(n, off, *outs)


def _sumsq_ranges(L, x, ranges, n_extra, out, scratch):
    flat = [v for r in ranges for v in r]
    return L.lib().vbx_sumsq_ranges(x.data_ptr(), _longs(flat), len(ranges), n_extra, out.data_ptr(), scratch.data_ptr(), st())


@pytest.mark.parametrize("case", RANGES_CASES, ids=lambda c: c.name)
def test_sumsq_ranges(L, case):
    x, scratch0 = oc.ranges_input(case)
    x = x.to(dev)
    outs = []
    for _ in range(2):
        out, scratch = _out(), scratch0.to(dev)
        assert _sumsq_ranges(L, x, case.ranges, case.n_extra, out, scratch) == 0, L.lib().vbx_last_error().decode()
        torch.cuda.synchronize()
        assert int(oc.bits(out.cpu())[1]) == oc.SENTINEL[torch.float32][1]
        assert torch.equal(oc.bits(scratch.cpu()[1024:]), oc.bits(scratch0[1024:]))  # the extra terms and the guard behind them: read only
        outs.append(out.cpu()[:1])
    oc.check_ranges(case, *outs)


@pytest.mark.parametrize("sh", GRAM_CASES, ids=oc.gram_name)
def test_sumsq_adaln_factors(L, sh):
    Ln, B, J4, Th = sh
    dada, temb = _operands(*oc.gram_inputs(sh))
    outs = []
    for _ in range(2):
        out = oc.sentinel(Ln * B * B + 8, torch.float32).to(dev)
        rc = L.lib().vbx_sumsq_adaln_factors(_ptr(*dada), _ptr(*temb), Ln, B, J4, Th, out.data_ptr(), st())
        assert rc == 0, L.lib().vbx_last_error().decode()
        torch.cuda.synchronize()
        assert bool((oc.bits(out.cpu())[Ln * B * B:] == oc.SENTINEL[torch.float32][1]).all())
        outs.append(out.cpu()[: Ln * B * B])
    oc.check_gram(sh, *outs)


@pytest.mark.parametrize("case", CLIP_CASES, ids=oc.clip_name)
def test_clip_coef(L, case):
    ss, max_norm, inv_world = case
    coef = oc.sentinel(3, torch.float32).to(dev)
    L.call("vbx_clip_coef", torch.tensor([ss], device=dev), max_norm, inv_world, coef, st())
    torch.cuda.synchronize()
    assert int(oc.bits(coef.cpu())[2]) == oc.SENTINEL[torch.float32][1]
    oc.check_clip(case, coef.cpu()[:2])


def test_host_refusals_launch_nothing(L):
    """Arguments outside the contracts of include/vbx.h are answered with an error code; no output is written."""
    lib = L.lib()
    x = torch.ones(1024, device=dev)
    out, scratch = _out(), torch.zeros(1024 + 8, device=dev)
    assert _sumsq_ranges(L, x, ((2, 10),), 0, out, scratch) != 0  # a range bound that is no multiple of 4 floats
    assert _sumsq_ranges(L, x, ((0, 8), (12, 18)), 0, out, scratch) != 0
    assert _sumsq_ranges(L, x, tuple((8 * i, 8 * i + 4) for i in range(65)), 0, out, scratch) != 0  # n > 64
    assert _sumsq_ranges(L, x[1:], ((0, 8),), 0, out, scratch) != 0  # a base that is not 16-byte aligned
    torch.cuda.synchronize()
    sent = oc.SENTINEL[torch.float32][1]
    assert bool((oc.bits(out.cpu()) == sent).all())
    assert _sumsq_ranges(L, x, ((0, 8),), 0, out, scratch) == 0  # (the same call within the contract is served)
    torch.cuda.synchronize()
    assert float(out.cpu()[0]) == 8.0
    lay = oc.factor_layout(2, 8, 6)
    state = {k: oc.sentinel(lay["n"] + oc.GUARD, torch.float32).to(dev) for k in "pmv"}
    dada, temb = torch.ones(2 * 65 * 8 + 8, device=dev), torch.ones(65 * 8 + 8, device=dev)
    none = (C.c_void_p * 2)(None, None)

    def adam(off, Th, B=3):
        return lib.vbx_adam_adaln_factors(state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), _longs(off), none,
                                          dada.data_ptr(), temb.data_ptr(), 2, B, 8, Th, *HYPER, 1, None, st())

    assert adam(lay["w_off"], 6) != 0
    assert adam([lay["w_off"][0] + 2, lay["w_off"][1]], 4) != 0  # a weight offset that is not 16-byte aligned
    dw = oc.sentinel(8 * 8, torch.float32).to(dev)
    assert lib.vbx_adaln_expand_dw(temb.data_ptr(), dada.data_ptr(), dw.data_ptr(), 3, 6, 8, 0, st()) != 0
    terms = oc.sentinel(2 * 65 * 65, torch.float32).to(dev)
    assert lib.vbx_sumsq_adaln_factors(dada.data_ptr(), temb.data_ptr(), 2, 65, 8, 8, terms.data_ptr(), st()) != 0  # B > 64
    torch.cuda.synchronize()
    for t in (dw, terms, *state.values()):
        assert bool((oc.bits(t.cpu()) == sent).all())


# ----------------------------------------------------------------------------- E. the chain
def test_clip_adam_chain(L):
    """Gram terms, vbx_sumsq_ranges with the terms as extras, vbx_clip_coef, then both Adam launches with gscale = coef: three steps on
    one flat buffer, each compared with fp64 clip_grad_norm_ + Adam on the materialised gradient from the device's own previous state."""
    table, lay, ranges = oc.chain_layout()
    nt = oc.chain_nterms()
    state = {k: t.to(dev) for k, t in oc.chain_initial().items()}
    dst = {n: t.to(dev) for n, t in oc.new_dst(table).items()}
    fdst = {n: t.to(dev) for n, t in oc.new_factor_dst(lay).items()}
    for step in range(1, CHAIN_STEPS + 1):
        g, dada, temb = oc.chain_grads(step)
        before = cpu(state)
        dada_d, temb_d = _operands(dada, temb)
        scratch = torch.full((1024 + nt + 8,), float("nan"), device=dev)
        ss, coef = _out(), oc.sentinel(3, torch.float32).to(dev)
        rc = L.lib().vbx_sumsq_adaln_factors(_ptr(*dada_d), _ptr(*temb_d), lay["L"], oc.CHAIN_B, lay["J4"], lay["Th"], _ptr(scratch, 1024), st())
        assert rc == 0, L.lib().vbx_last_error().decode()
        gd = g.to(dev)
        assert _sumsq_ranges(L, gd, ranges, nt, ss, scratch) == 0, L.lib().vbx_last_error().decode()
        L.call("vbx_clip_coef", ss, oc.CHAIN_MAX_NORM, 1.0, coef, st())
        _adam_packed(L, table, state, gd, dst, step, coef)
        _adam_factors(L, lay, state, dada_d, temb_d, fdst, oc.CHAIN_B, step, coef)
        got = cpu({**state, **dst, **fdst, "terms": scratch[1024: 1024 + nt], "sumsq": ss[:1], "coef": coef[:2]})
        oc.check_chain_step(step, before, got)


# ----------------------------------------------------------------------------- the table of a real model
@pytest.mark.parametrize("factors", [False, True], ids=["materialized", "factors"])
def test_model_segment_table_invariants(L, factors):
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=64, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False).to(dev)
    eng = vb.engine(2, 64, True)
    eng.bind_params()  # the table points into the packed arena of a bound model
    tab, nblocks = eng._adam_segments_host(factors)
    segs = [{f: (getattr(s, f) or 0) for f in oc.SEG_FIELDS} for s in tab]
    blocks = eng.adaln_factor_ranges() if factors else []
    assert len(blocks) == (2 if factors else 0)
    oc.check_segment_table(segs, nblocks, eng.fp.flat.numel(), blocks, (eng.wpack.data_ptr(), eng.wpack.data_ptr() + eng.wpack.numel()))
