"""The length-aware attention entry points -- vbx_attn_fwd_lens, vbx_attn_bwd_lens, vbx_attn_bwd_fused_lens, vbx_attn_fwd_segs -- against
the fp64 restatement (restate.attend with the prefix mask n < key_lens[b], autograd with dout zeroed behind the prefix; per segment on
the segment's live rows alone), at the inputs where the boundary decides the result (attn_check.edge_inputs: the last live key holds
>= 0.02 of every softmax, every dead key is a trap of +4 nats with v = 64).

The other suites compare these kernels with the masked kernels bit for bit (test_sample_lens_gpu.py, test_train_lens_gpu.py,
test_sample_pack_gpu.py) at Np 216 and 272; the masked kernels meet fp64 in test_attn_edges_gpu.py under masks that are no prefix.  Here
each instantiation meets fp64 itself, at its own key bound kend, tile count ceil(kend / 64), DMA clamp, dead-tile early-out and tail
role: Np 1 .. 1040 with kend on, before and behind the seams of the 64-key and 128-row tiles and in the <= 16-row tail tile, 17 ring
tiles, B * H = 9 and 17 (padded work ids).  tests/test_attn_check_cpu.py shows on CPU that every check used here rejects a planted fault.

Every output buffer is NaN-filled with a guard row; each entry point runs twice and with mask = the prefix bytes and mask = NULL, and
all of them must agree bit for bit.  Bounds: attn_check.BOUNDS lens / lens_qknorm / lens_fused / segs, inherited from the masked
kernels; measured values of one run in profiles/attn_lens_edges_measured.json (ATTN_CHECK_LOG).
"""
import pytest
import torch

from attn_check import (BOUNDS, LENS_CASES, SEGS_CASES, Checks, L_tiles, all_nan, bf, check_lens_bwd, check_lens_fused, check_lens_fwd,
                        check_segs, edge_inputs, heads, lens_case_id, lens_case_seed, lens_reference, prefix_mask, q_operand, q_prescale,
                        same_bits, segs_inputs, segs_reference)
from test_attn_edges_gpu import L, dev, nans, st  # noqa: F401  (L is the module fixture)

pytestmark = pytest.mark.gpu


class LensCase:
    """One set of edge inputs, its fp64 reference (computed once for the forward, the unfused and the fused backward) and the device
    copies; every launch writes NaN-filled buffers with one guard row past the end."""

    def __init__(self, L, case):
        self.B, self.H, self.Np, self.kl, self.regime = case
        self.I = self.H * 64
        inp = self.inp = edge_inputs(*case, seed=lens_case_seed(case))
        c = self.c = L.lib().vbx_attn_q_prescale(inp["scale"])
        self.ref = lens_reference(inp, c)
        self.scale = inp["scale"]
        self.qd, self.kd, self.vd = q_operand(inp["q16"], c)[0].to(dev), inp["k16"].to(dev), inp["v16"].to(dev)
        self.qb, self.kb, self.vb = (bf(inp[n].float()).to(dev) for n in ("q16", "k16", "v16"))
        self.doutd = inp["dout"].to(dev)
        self.kld = torch.tensor(self.kl, dtype=torch.int32, device=dev)
        self.md = prefix_mask(self.kl, self.Np).contiguous().to(dev)
        f = inp["fused"]
        self.rn = (1 / f["pre"].norm(dim=-1)).float().to(dev)
        self.gam, self.rc, self.rs = f["gam"].float().to(dev), f["rc"].float().to(dev), f["rs"].float().to(dev)

    def fwd(self, L, mask):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        o16, ob, lse = nans((B * Np + 1, I), torch.float16), nans((B * Np + 1, I), torch.bfloat16), nans((B * H * Np + 1,), torch.float32)
        L.call("vbx_attn_fwd_lens", self.qd, self.kd, self.vd, mask, self.kld, o16, ob, lse, B, H, Np, self.scale, st())
        torch.cuda.synchronize()
        return o16, ob, lse

    def bwd(self, L, o16, lse, mask):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        dq, dk = nans((B * H * Np + 1, 64), torch.float32), nans((B * H * Np + 1, 64), torch.float32)
        d = nans((B * Np + 1, 3 * I), torch.bfloat16)
        delta = torch.empty(B, H, Np, device=dev)
        L.call("vbx_attn_bwd_lens", self.qd, self.kd, self.qb, self.kb, self.vb, mask, self.kld, o16, 1, self.doutd, lse, delta, dq, dk,
               d[:, 2 * I:].data_ptr(), 3 * I, B, H, Np, self.scale, None, st())
        torch.cuda.synchronize()
        return dq, dk, d

    def bwd_fused(self, L, o16, lse, mask, qk_scale):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        d = nans((B * Np + 1, 3 * I), torch.bfloat16)
        gp = nans((2 * B * L.lib().vbx_attn_bwd_fused_tiles(Np) + 1, H, 64), torch.float32)
        delta = torch.empty(B, H, Np, device=dev)
        L.call("vbx_attn_bwd_fused_lens", self.qd, self.kd, self.qb, self.kb, self.vb, mask, self.kld, o16, 1, self.doutd, lse, delta,
               self.rn[0], self.rn[1], self.gam[0], self.gam[1], self.rc, self.rs, qk_scale, d, 3 * I, gp, B, H, Np, self.scale, None, st())
        torch.cuda.synchronize()
        return d, gp

    # ---- the buffers in the layout of the checks; guard rows judged here
    def fwd_views(self, chk, o16, ob, lse):
        B, H, Np = self.B, self.H, self.Np
        n = B * Np
        chk.true("out16 / out_bf16 / lse guard rows untouched", all_nan(o16[n]) and all_nan(ob[n]) and all_nan(lse[B * H * Np:]))
        return dict(out16=heads(o16[:n], B, Np, H), out_bf16=heads(ob[:n], B, Np, H), lse=lse[:B * H * Np].view(B, H, Np))

    def bwd_views(self, chk, dq, dk, d):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        n, m = B * Np, B * H * Np
        chk.true("dq / dk guard rows untouched", all_nan(dq[m]) and all_nan(dk[m]))
        chk.true("dv: q and k blocks and the guard row untouched", all_nan(d[:n, :2 * I]) and all_nan(d[n]))
        return dict(dq=dq[:m].view(B, H, Np, 64), dk=dk[:m].view(B, H, Np, 64), dv=heads(d[:n, 2 * I:], B, Np, H))

    def fused_views(self, chk, d, gp, qknorm, tag):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        n, tiles = B * Np, L_tiles(Np)
        chk.true(f"d(qkv){tag} guard row untouched", all_nan(d[n]))
        if qknorm:
            chk.true(f"gpart{tag} guard record untouched", all_nan(gp[2 * B * tiles]))
        else:
            chk.true(f"gpart{tag}: no record is written without qk-norm", all_nan(gp))
        return dict(dpre_q=heads(d[:n, :I], B, Np, H), dpre_k=heads(d[:n, I:2 * I], B, Np, H), dv=heads(d[:n, 2 * I:], B, Np, H),
                    gpart=gp[:2 * B * tiles].view(2, B, tiles, H, 64))


@pytest.mark.parametrize("case", LENS_CASES, ids=[lens_case_id(c) for c in LENS_CASES])
def test_attn_lens_edges(L, case):
    """vbx_attn_fwd_lens, vbx_attn_bwd_lens and vbx_attn_bwd_fused_lens (qk-norm + rotary; rotary alone at Np 145 and 1040) on one set
    of edge inputs against one fp64 reference."""
    c = LensCase(L, case)
    kl, Np, qk = c.kl, c.Np, c.regime == "edge_qknorm"
    chk = Checks("lens " + lens_case_id(case))
    chk.true("vbx_attn_q_prescale is scale * log2(e) in fp32 (the share condition was judged with it)", c.c == q_prescale(c.scale))
    bounds = BOUNDS["lens_qknorm" if qk else "lens"]
    row_floor = bounds.get("floor") if qk else None  # one-hot softmax: the boundary row of dk is judged against a floor, as its tiles are
    # ---- forward
    o16, ob, lse = c.fwd(L, c.md)
    check_lens_fwd(chk, kl, c.fwd_views(chk, o16, ob, lse), c.ref, bounds)
    for what, m in (("repeats", c.md), ("with mask = NULL gives the same bits", None)):
        again = c.fwd(L, m)
        chk.true("forward " + what, all(same_bits(a, b) for a, b in zip((o16, ob, lse), again)))
    # ---- unfused backward
    dq, dk, d = c.bwd(L, o16, lse, c.md)
    check_lens_bwd(chk, kl, c.bwd_views(chk, dq, dk, d), c.ref, bounds, row_floor=row_floor)
    for what, m in (("repeats", c.md), ("with mask = NULL gives the same bits", None)):
        again = c.bwd(L, o16, lse, m)
        chk.true("backward " + what, all(same_bits(a, b) for a, b in zip((dq, dk, d), again)))
    # ---- fused backward
    for qk_scale in (8.0, 0.0) if Np in (145, 1040) else (8.0,):
        tag = " (fused)" if qk_scale else " (fused, rotary only)"
        d, gp = c.bwd_fused(L, o16, lse, c.md, qk_scale)
        check_lens_fused(chk, kl, c.fused_views(chk, d, gp, qk_scale > 0, tag), c.ref, BOUNDS["lens_fused"], qknorm=qk_scale > 0, tag=tag,
                         row_floor=row_floor)
        for what, m in (("repeats", c.md), ("with mask = NULL gives the same bits", None)):
            again = c.bwd_fused(L, o16, lse, m, qk_scale)
            chk.true(f"fused backward{tag} " + what, same_bits(d, again[0]) and same_bits(gp, again[1]))
    chk.done()


@pytest.mark.parametrize("H,klens,extra", SEGS_CASES, ids=[f"H{H}-" + "_".join(map(str, k)) for H, k, _ in SEGS_CASES])
def test_attn_segs_edges(L, H, klens, extra):
    """vbx_attn_fwd_segs on one packed row of edge segments with `extra` trailing -1 tiles, every dead row of q, k and v NaN: live rows
    against the per-segment fp64 reference, dead rows and -1 tiles zero with lse 1e30, no NaN anywhere."""
    from voicebox_pytorch_amd import sample_pack as sp

    inp = segs_inputs(H, klens, extra)
    Mp, I = inp["Mp"], H * 64
    c = L.lib().vbx_attn_q_prescale(inp["scale"])
    ref = segs_reference(inp, c)
    tabs = [torch.tensor(t, dtype=torch.int32) for t in (inp["seg_start"], klens, inp["tile_seg"])]
    sp.check_tables(*tabs, Mp, len(klens))
    tabs = [t.to(dev) for t in tabs]
    qd, kd, vd = q_operand(inp["q16"], c)[0].to(dev), inp["k16"].to(dev), inp["v16"].to(dev)

    def run():
        o16, ob, lse = nans((Mp + 1, I), torch.float16), nans((Mp + 1, I), torch.bfloat16), nans((H * Mp + 1,), torch.float32)
        L.call("vbx_attn_fwd_segs", qd, kd, vd, *tabs, o16, ob, lse, H, Mp, inp["scale"], st())
        torch.cuda.synchronize()
        return o16, ob, lse

    chk = Checks(f"segs H={H} klens={klens}")
    o16, ob, lse = run()
    chk.true("out16 / out_bf16 / lse guard rows untouched", all_nan(o16[Mp]) and all_nan(ob[Mp]) and all_nan(lse[H * Mp:]))
    got = dict(out16=heads(o16[:Mp], 1, Mp, H), out_bf16=heads(ob[:Mp], 1, Mp, H), lse=lse[:H * Mp].view(1, H, Mp))
    check_segs(chk, inp, got, ref, BOUNDS["segs"])
    chk.true("segments repeat", all(same_bits(a, b) for a, b in zip((o16, ob, lse), run())))
    chk.done()
