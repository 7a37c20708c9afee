"""The per-tile error metric of the attention tests (tests/attn_check.py) on CPU: errors confined to one tail tile pass the global
bounds of tests/test_ops_gpu.py::test_attn_fwd_bwd and are rejected per tile; tiles whose reference is exactly zero must be exactly
zero.  Then the checks of the length-aware entry points (tests/test_attn_lens_edges_gpu.py): a torch stand-in of those kernels passes
every one of them under the bounds the GPU test uses, and each planted boundary fault is rejected by a named check."""
import math

import pytest
import torch

from attn_check import (BOUNDS, DEAD_LSE, LENS_CASES, SEGS_CASES, SHARE_MIN, Checks, L_tiles, _chain, _unrotate, attn_inputs, bf,
                        check_lens_bwd, check_lens_fused, check_lens_fwd, check_segs, edge_inputs, heads, lens_case_seed,
                        lens_reference, q_operand, q_prescale, rel_err, segs_inputs, segs_reference, tile_errors, worst_tile)
from oracle import restate


def _confine(ref, b, h, rows, frac, seed):
    """ref with an error of relative size `frac` added to rows `rows` of (b, h) only."""
    got = ref.clone()
    tile = ref[b, h, rows]
    u = torch.randn(tile.shape, generator=torch.Generator().manual_seed(seed), dtype=ref.dtype)
    got[b, h, rows] = tile + frac * tile.norm() * u / u.norm()
    return got


def test_forward_tail_error_hides_under_the_global_bound():
    """2 % on one head's 5-row tail tile at (B, H, Np) = (1, 2, 1029), the reference's temperature."""
    q, k, v = (t.double() for t in attn_inputs(1, 2, 1029, seed=1031))
    ref = restate.attend(q, k, v, scale=10.0)
    got = _confine(ref, 0, 1, slice(1024, 1029), 0.02, seed=1)
    assert rel_err(got, ref) < 1.5e-3, rel_err(got, ref)  # test_attn_fwd_bwd's out16 bound: accepted
    err, idx = worst_tile(tile_errors(got, ref))
    assert idx == (0, 1, 8) and abs(err - 0.02) < 1e-9, (err, idx)
    assert err > BOUNDS["qknorm"]["out16_tile"] and err > BOUNDS["spread"]["out16_tile"]  # rejected per tile
    assert float(tile_errors(got, ref)[0, 0].max()) == 0.0  # the other head is untouched


def test_dq_tail_error_hides_under_the_global_bound():
    """30 % on one (b, h)'s 16-row dq tail tile at (B, H, Np) = (2, 2, 1040)."""
    q, k, v = (t.double().requires_grad_(True) for t in attn_inputs(2, 2, 1040, seed=1042))
    out = restate.attend(q, k, v, scale=10.0)
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=out.dtype) * 1e-3)
    ref = q.grad
    got = _confine(ref, 1, 0, slice(1024, 1040), 0.3, seed=2)
    assert rel_err(got, ref) < 2e-2, rel_err(got, ref)  # test_attn_fwd_bwd's dq bound: accepted
    err, idx = worst_tile(tile_errors(got, ref))
    assert idx == (1, 0, 8) and abs(err - 0.3) < 1e-9, (err, idx)
    assert err > BOUNDS["spread"]["dq_tile"]
    # the qk-norm group measures dq tiles against half the typical tile norm (one-hot rows): the error is still rejected there
    err_f, idx_f = worst_tile(tile_errors(got, ref, floor=BOUNDS["qknorm"]["floor"]["dq"]))
    assert idx_f == (1, 0, 8) and err_f > BOUNDS["qknorm"]["dq_tile"], (err_f, idx_f)


def test_tile_errors_zero_reference_tiles():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(2, 3, 300, 64, generator=g, dtype=torch.float64)
    ref[0, 1, 128:256] = 0  # a masked key tile: dk / dv of masked keys are exactly zero
    ref[1] = 0  # a fully masked batch: its dq and dk
    got = ref.clone()
    e = tile_errors(got, ref)
    assert e.shape == (2, 3, 3) and float(e.max()) == 0.0
    got[0, 1, 200, 5] = 1e-30  # the smallest departure from an exactly-zero reference tile is rejected
    e = tile_errors(got, ref)
    assert math.isinf(float(e[0, 1, 1])) and float(e[0, 1, 0]) == 0.0
    got = ref.clone()
    got[1, 2, 299] = -0.0  # signed zero is zero
    assert float(tile_errors(got, ref).max()) == 0.0
    # a NEARLY zero tile is measured against the floor 1e-3 * rms(ref) * sqrt(n): an error far below the floor stays small
    ref2 = ref.clone()
    ref2[0, 0, :128] = 1e-12
    got2 = ref2.clone()
    got2[0, 0, :128] += 1e-12
    e2 = float(tile_errors(got2, ref2)[0, 0, 0])
    assert 0 < e2 < 1e-6, e2
    # the last, partial tile is measured over its own rows (44 here); NaN fails a Checks bound
    got3 = ref.clone()
    got3[0, 0, 256:] *= 1.01
    assert abs(float(tile_errors(got3, ref)[0, 0, 2]) - 0.01) < 1e-12
    got3[0, 2, 7, 7] = math.nan
    chk = Checks("nan")
    chk.tiles("x", got3, ref, 1.0)
    assert chk.bad


# ----------------------------------------------------------------------------- the length-aware checks (tests/test_attn_lens_edges_gpu.py)
# A torch stand-in of vbx_attn_fwd_lens / vbx_attn_bwd_lens / vbx_attn_bwd_fused_lens / vbx_attn_fwd_segs at the kernels' precision:
# fp32 sums over fp16-rounded q, k, v, an fp16 P in the forward, fp16 / bf16 outputs; bf16 dO, v, q, k, P and dS in the backward.  It
# walks the keys in 64-key tiles up to ceil(klen / 64), writes into NaN-filled buffers, zero-fills wholly dead 128-row tiles, and
# takes a planted fault.  The clean stand-in must pass every check under the bounds the GPU test uses; every fault must fail one.
FWD_FAULTS = ("fwd_skip_tail", "leak_key", "drop_last_key", "klen_of_next_row", "dead_tile_nan", "dead_tile_masked")


def _rows_fwd(qs, k, v, kend, ntiles):
    """Online softmax of the query rows qs [H, nq, 64] over keys k, v [H, nk, 64] in 64-key tiles, keys >= kend masked."""
    Hh, nq = qs.shape[:2]
    m = torch.full((Hh, nq), -math.inf)
    l, o = torch.zeros(Hh, nq), torch.zeros(Hh, nq, 64)
    for kt in range(ntiles):
        k0, k1 = kt * 64, min(kt * 64 + 64, k.shape[1])
        s = qs @ k[:, k0:k1].transpose(1, 2)
        s = s.masked_fill(torch.arange(k0, k1)[None, None, :] >= kend, -math.inf)
        m_new = torch.maximum(m, s.amax(-1))
        m_use = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
        alpha, p = torch.exp2(m - m_use), torch.exp2(s - m_use[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p.half().float() @ v[:, k0:k1]
        m = m_new
    live = l > 0
    out = torch.where(live[..., None], o / l.clamp(min=1e-38)[..., None], torch.zeros_like(o))
    return out, torch.where(live, m + torch.log2(l.clamp(min=1e-38)), torch.full_like(l, DEAD_LSE))


def _klen(key_lens, b, fault):
    kl = key_lens[(b + 1) % len(key_lens)] if fault == "klen_of_next_row" else key_lens[b]
    return kl + (fault == "leak_key") - (fault == "drop_last_key")


def standin_fwd(inp, fault=None):
    B, H, Np = inp["B"], inp["H"], inp["Np"]
    qs = q_operand(inp["q16"], q_prescale(inp["scale"]))[0].float()
    k, v = inp["k16"].float(), inp["v16"].float()
    out = torch.full((B, H, Np, 64), math.nan)
    lse = torch.full((B, H, Np), math.nan)
    for b in range(B):
        kend = min(max(_klen(inp["key_lens"], b, fault), 0), Np)
        ntiles = kend // 64 if fault == "fwd_skip_tail" else -(-kend // 64)
        for r0 in range(0, Np, 128):
            rows = slice(r0, min(r0 + 128, Np))
            if r0 >= kend and fault == "dead_tile_nan":
                continue
            if r0 >= kend and fault != "dead_tile_masked":
                out[b, :, rows], lse[b, :, rows] = 0.0, DEAD_LSE
            else:
                out[b, :, rows], lse[b, :, rows] = _rows_fwd(qs[b, :, rows], k[b], v[b], kend, ntiles)
    return dict(out16=out.half(), out_bf16=out.bfloat16(), lse=lse)


def standin_bwd(inp, fwd, fault=None):
    """dq, dk fp32 and dv bf16 [B, H, Np, 64] from the forward's fp16 output and lse (delta = rowsum(dO * O))."""
    B, H, Np, scale = inp["B"], inp["H"], inp["Np"], inp["scale"]
    qs = q_operand(inp["q16"], q_prescale(scale))[0].float()
    k16 = inp["k16"].float()
    qb, kb, vb = (bf(inp[n].float()).float() for n in ("q16", "k16", "v16"))
    dO = heads(inp["dout"].float(), B, Np, H)
    dq, dk, dv = (torch.full((B, H, Np, 64), math.nan) for _ in range(3))
    for b in range(B):
        kend = min(max(_klen(inp["key_lens"], b, fault), 1), Np)
        nt = -(-kend // 64)
        kq = min((kend // 64 if fault == "dq_skip_tail" else nt) * 64, Np)  # keys the dq role walks
        qk = min((kend // 64 if fault == "dkv_skip_tail" else nt) * 64, Np)  # queries the dk / dv role walks
        delta = (dO[b] * fwd["out16"][b].float()).sum(-1)
        P = torch.exp2(qs[b] @ k16[b].transpose(1, 2) - fwd["lse"][b][..., None])
        P = P.masked_fill(torch.arange(Np)[None, None, :] >= kend, 0.0)
        dS = bf(P * (dO[b] @ vb[b].transpose(1, 2) - delta[..., None])).float()
        dq[b] = scale * (dS[:, :, :kq] @ kb[b, :, :kq])
        dk[b] = scale * (dS[:, :qk].transpose(1, 2) @ qb[b, :, :qk])
        dv[b] = bf(P[:, :qk]).float().transpose(1, 2) @ dO[b, :, :qk]
        for r0 in range(0, Np, 128):
            rows = slice(r0, min(r0 + 128, Np))
            if r0 >= kend:
                for t in (dq, dk, dv):
                    t[b, :, rows] = math.nan if fault == "dead_tile_nan" else 0.0
            elif r0 + 128 > kend and fault == "dq_dead_rows_nonzero":
                dq[b, :, kend:rows.stop] = 1e-9
    return dict(dq=dq, dk=dk, dv=dv.bfloat16())


def standin_fused(inp, bwd, fault=None):
    """The fp32 backward of rotary(l2norm(pre) * 8 * gamma) on the stand-in's dq, dk: dpre_q, dpre_k (bf16) and the gpart records."""
    B, H, Np, f = inp["B"], inp["H"], inp["Np"], inp["fused"]
    pre = f["pre"].clone().requires_grad_(True)
    fr, tiles = f["fr"].float(), L_tiles(Np)
    grads = [torch.nan_to_num(bwd["dq"]), torch.nan_to_num(bwd["dk"])]
    torch.autograd.backward(_chain(fr, pre, f["gam"]), grads)
    gp = torch.full((2, B * tiles, H, 64), math.nan)
    for w in range(2):
        rec = _unrotate(fr, grads[w]) * restate.l2norm_scale(f["pre"][w], 64)  # [B, H, Np, 64]: d(gamma) per row
        for b, kl in enumerate(inp["key_lens"]):
            mine = L_tiles(kl) if fault == "gpart_tiles_by_klen" else tiles
            for t in range(tiles):
                dead = t * 128 >= kl
                if (dead and fault == "gpart_dead_not_zeroed") or t >= mine:
                    continue
                gp[w, b * mine + t] = 0.0 if dead else rec[b, :, t * 128:(t + 1) * 128].sum(1)
    return dict(dpre_q=pre.grad[0].bfloat16(), dpre_k=pre.grad[1].bfloat16(), dv=bwd["dv"], gpart=gp.view(2, B, tiles, H, 64))


def standin_segs(inp, fault=None):
    H, Mp, klens, starts = inp["H"], inp["Mp"], inp["klens"], inp["seg_start"]
    qs = q_operand(inp["q16"], q_prescale(inp["scale"]))[0].float()[0]
    k, v = inp["k16"].float()[0], inp["v16"].float()[0]
    out, lse = torch.full((1, H, Mp, 64), math.nan), torch.full((1, H, Mp), math.nan)
    for t, seg in enumerate(inp["tile_seg"]):
        rows = slice(t * 128, t * 128 + 128)
        if seg < 0:
            out[0, :, rows], lse[0, :, rows] = 0.0, DEAD_LSE
            continue
        kend = klens[(seg + 1) % len(klens)] if fault == "klen_of_next_segment" else klens[seg]
        base = 0 if fault == "keys_from_row_0" else starts[seg]
        o, l = _rows_fwd(qs[:, rows], k[:, base:base + kend], v[:, base:base + kend], kend, -(-kend // 64))
        qdead = torch.arange(rows.start, rows.stop) - starts[seg] >= klens[seg]
        out[0, :, rows] = torch.where(qdead[None, :, None], torch.zeros_like(o), o)
        lse[0, :, rows] = torch.where(qdead[None, :], torch.full_like(l, DEAD_LSE), l)
    return dict(out16=out.half(), out_bf16=out.bfloat16(), lse=lse)


STANDIN_CASES = {145: (3, 3, 145, (2, 17, 130), "edge"), 1040: (3, 3, 1040, (1, 1025, 1040), "edge"),
                 "145-qknorm": (3, 3, 145, (2, 17, 130), "edge_qknorm"), "1040-qknorm": (3, 3, 1040, (1, 1025, 1040), "edge_qknorm")}
_BUILT = {}


def _case(key):
    if key not in _BUILT:
        c = STANDIN_CASES[key]
        inp = edge_inputs(*c, seed=lens_case_seed(c))
        _BUILT[key] = (inp, lens_reference(inp))
    return _BUILT[key]


def _run_lens(key, fault):
    """every check of the three length-aware entry points on the stand-in, under the bounds and the row floor the GPU test uses for the
    case's regime -> the Checks"""
    inp, ref = _case(key)
    kl, qk = inp["key_lens"], STANDIN_CASES[key][4] == "edge_qknorm"
    bounds = BOUNDS["lens_qknorm" if qk else "lens"]
    row_floor = bounds.get("floor") if qk else None
    fwd = standin_fwd(inp, fault if fault in FWD_FAULTS else None)
    chk = Checks(f"stand-in {key} fault={fault}")
    check_lens_fwd(chk, kl, fwd, ref, bounds)
    bwd = standin_bwd(inp, standin_fwd(inp, fault if fault in ("leak_key", "drop_last_key", "klen_of_next_row") else None), fault)
    check_lens_bwd(chk, kl, bwd, ref, bounds, row_floor=row_floor)
    check_lens_fused(chk, kl, standin_fused(inp, bwd, fault), ref, BOUNDS["lens_fused"], row_floor=row_floor)
    return chk


def test_every_length_aware_case_meets_the_share_condition():
    """edge_inputs asserts in fp64 that the last live key holds >= 0.02 of every live query's softmax: every GPU case is built here."""
    for c in LENS_CASES:
        inp = edge_inputs(*c, seed=lens_case_seed(c))
        assert inp["share"] >= (SHARE_MIN if c[4] == "edge" else 0), (c, inp["share"])
        kl = torch.tensor(c[3])
        dead = ~(torch.arange(c[2])[None] < kl[:, None])
        assert bool((inp["dout"].view(c[0], c[2], -1)[dead] == 0).all()) and bool((inp["v16"].permute(0, 2, 1, 3)[dead] == 64).all())
    for H, klens, extra in SEGS_CASES:
        inp = segs_inputs(H, klens, extra)
        live = torch.zeros(inp["Mp"], dtype=torch.bool)
        for s0, n in zip(inp["seg_start"], klens):
            live[s0:s0 + n] = True
        for name in ("q16", "k16", "v16"):  # NaN exactly on the dead rows
            assert bool(torch.isnan(inp[name][0, :, ~live]).all()) and not bool(torch.isnan(inp[name][0, :, live]).any())


@pytest.mark.parametrize("Np", list(STANDIN_CASES))
def test_the_clean_stand_in_passes_every_length_aware_check(Np):
    chk = _run_lens(Np, None)
    assert not chk.bad, chk.bad
    assert len(chk.seen) >= 30  # forward 8, unfused backward 11, fused backward 14 and its gpart checks


# fault -> a check that must reject it (part of its name), on both cases
LENS_FAULTS = {
    "fwd_skip_tail": "out16",                   # forward: ntiles = klen // 64, the last partial key tile is skipped
    "dq_skip_tail": "dq",                       # the same in the dq sum
    "dkv_skip_tail": "dk",                      # the same in the dk / dv sum (its last partial QUERY tile)
    "leak_key": "out16",                        # key klen is included: the trap leaks
    "drop_last_key": "boundary row",            # key klen - 1 is excluded
    "klen_of_next_row": "out16",                # key_lens of batch row (b + 1) % B
    "dead_tile_nan": "no NaN",                  # a wholly dead tile keeps the buffer's NaN
    "dead_tile_masked": "wholly dead tiles",    # ... or is written with the masked kernel's nonzero values
    "dq_dead_rows_nonzero": "dq: rows >= key_lens[b] are exactly 0",
    "gpart_dead_not_zeroed": "gpart (fused): no NaN",
    "gpart_tiles_by_klen": "gpart (fused)",     # ceil(klen / 128) records per batch row instead of ceil(Np / 128)
}


@pytest.mark.parametrize("Np", [145, 1040])
@pytest.mark.parametrize("fault", sorted(LENS_FAULTS))
def test_a_planted_length_fault_is_rejected(fault, Np):
    chk = _run_lens(Np, fault)
    assert any(LENS_FAULTS[fault] in b for b in chk.bad), (fault, chk.bad)


@pytest.mark.parametrize("fault,want", [("drop_last_key", "dv boundary row"), ("leak_key", "out16"), ("dkv_skip_tail", "dv")])
def test_the_one_hot_regime_still_rejects_the_boundary_faults(fault, want):
    """edge_qknorm judges the boundary row of dk against a floor (its reference cancels); the row of dv and the trap still decide."""
    chk = _run_lens("145-qknorm", fault)
    assert any(want in b for b in chk.bad), (fault, chk.bad)


def test_the_segment_checks_pass_clean_and_reject_planted_faults():
    inp = segs_inputs(3, (1, 64, 65, 129, 1025), 1)
    ref = segs_reference(inp)
    for fault, want in ((None, None), ("keys_from_row_0", "out16"), ("klen_of_next_segment", "out16")):
        chk = Checks(f"segments stand-in fault={fault}")
        check_segs(chk, inp, standin_segs(inp, fault), ref, BOUNDS["segs"])
        if fault is None:
            assert not chk.bad, chk.bad
        else:
            assert any(want in b for b in chk.bad), (fault, chk.bad)
    # a dead row or a -1 tile that is not zero-filled, and a NaN taken from a dead input row
    clean = standin_segs(inp)
    for name, row, val, want in (("out16", 1, 0.5, "dead rows"), ("lse", inp["Mp"] - 1, 3.0, "dead rows"), ("out_bf16", 70, math.nan, "no NaN")):
        got = {k: v.clone() for k, v in clean.items()}
        got[name][0, 0, row] = val
        chk = Checks("segments stand-in, one dead row")
        check_segs(chk, inp, got, ref, BOUNDS["segs"])
        assert any(want in b for b in chk.bad), (name, chk.bad)


def test_tile_errors_lse_axis():
    ref = torch.linspace(1, 2, 2 * 2 * 1029, dtype=torch.float64).view(2, 2, 1029)
    got = ref.clone()
    got[1, 1, 1025] += 1e-2
    e = tile_errors(got, ref, axis=-1)
    assert e.shape == (2, 2, 9)
    assert worst_tile(e)[1] == (1, 1, 8) and float(e[0].max()) == 0.0
