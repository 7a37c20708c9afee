"""GPU: a layer's weight gradients on the side stream (vbx_wgrad_overlap, csrc/wgrad_overlap_plan.hpp) against the in-line order.

Same kernels, same operands, same reduction order: the flat gradient and the slab reduce's sum-of-squares partials must be
BIT-identical however the two streams interleave.  vbx_wgrad_overlap_delay holds either stream back, so that a missing wait of the
schedule reads a buffer before it is written (side stream early) or after it was overwritten (side stream late) even at these sizes.
Shapes: depth 4 uses every copy of the layer-indexed buffers (two, and three for dxb) and the start-of-layer wait at two layers;
72 and 112 frames leave partial tiles; dim 512 takes the weight-stationary GEMM and the lean norm route of the flagship shape.
(The dim-512 case was asked for at depth 3; VoiceBox, like the reference, refuses an odd depth, so it runs at depth 4 -- one more
layer of the same checks.  The schedule at L = 3, and 1, 2, 5, 12, 24, is checked on the host: test_wgrad_overlap_cpu.py.)"""
import ctypes as C
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

CASES = {"dim128": dict(dim=128, heads=2, depth=4, B=2, N=72), "dim512": dict(dim=512, heads=8, depth=4, B=2, N=112)}


class ProfEntry(C.Structure):
    _fields_ = [("label", C.c_char * 24), ("calls", C.c_int), ("total_us", C.c_float)]


class _Case:
    """One model, one forward; backward(mode) re-runs the backward of that forward into a sentinel-filled gradient buffer."""

    def __init__(self, dim, heads, depth, B, N):
        import voicebox_pytorch_amd as vbx
        from voicebox_pytorch_amd import _lib
        from voicebox_pytorch_amd.dp import TrainStep
        from voicebox_pytorch_amd.masks import rng_override
        from oracle import restate

        self.lib, self.L = _lib.lib(), depth
        cfg = restate.Cfg(dim=dim, depth=depth, heads=heads, dim_head=64)
        state = restate.init_state_dict(cfg, seed=11)
        for k in state:  # the adaLN projections are zero-initialised: move them, so that their gradients carry signal
            if ".to_gamma." in k or ".to_beta." in k:
                state[k] = state[k] + 0.05 * torch.randn(state[k].shape, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()) % 1000))
        g = torch.Generator().manual_seed(1234 + dim)
        x1 = torch.randn(B, N, dim, generator=g)
        draws = dict(x0=torch.randn(B, N, dim, generator=g), times=torch.rand(B, generator=g),
                     frac_lengths=0.7 + 0.3 * torch.rand(B, generator=g), rand=torch.rand(B, generator=g))
        vb = vbx.VoiceBox(dim=dim, num_cond_tokens=5, depth=depth, dim_head=64, heads=heads, condition_on_text=False)
        vb.load_state_dict(state, strict=False)
        self.ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev)), lr=1e-3, max_grad_norm=0.5)
        assert self.ts.adaln_factors_apply()
        self.lib.vbx_wgrad_overlap(0)
        with rng_override(**draws):
            self.ts._forward_backward(x1.to(dev), None, None, on_stage=None, adaln_factors=True)  # the one forward
        self.eng = self.ts._last_eng
        nsq = self.eng.sq_partials_info()[0]
        assert nsq > 0
        self.scratch = torch.zeros(self.eng.sumsq_scratch_floats(True), device=dev)
        self.sq = self.scratch[-nsq:]
        assert self.sq.data_ptr() == self.eng.sq_partials_ptr(self.scratch)
        torch.cuda.synchronize()
        self.ref = self.backward(overlap=0)

    def submit(self, on_stage=None):
        self.ts.gflat.fill_(7.0)
        self.sq.fill_(-1.0)
        self.eng.backward(self.ts.gflat, gscale=None, on_stage=on_stage, adaln_factors=True, sq_partials=None if on_stage else self.eng.sq_partials_ptr(self.scratch))

    def backward(self, overlap, side_us=0.0, main_us=0.0, twice=False, on_stage=None):
        lib = self.lib
        assert lib.vbx_wgrad_overlap(overlap) == 0 and lib.vbx_wgrad_overlap_delay(side_us, main_us) == 0
        forks = lib.vbx_wgrad_overlap_forks()
        try:
            self.submit(on_stage)
            if twice:  # no host synchronise in between: the second head must not run under the first backward's side stream
                self.submit(on_stage)
            torch.cuda.synchronize()
        finally:
            lib.vbx_wgrad_overlap_delay(0.0, 0.0)
            lib.vbx_wgrad_overlap(1)
        self.forks = lib.vbx_wgrad_overlap_forks() - forks
        return self.ts.gflat.clone(), self.sq.clone()


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    c = _Case(**CASES[request.param])
    yield c
    c.lib.vbx_wgrad_overlap_delay(0.0, 0.0)
    c.lib.vbx_wgrad_overlap(1)


def _same(case, got):
    g, sq = got
    gr, sqr = case.ref
    assert torch.isfinite(gr[gr != 7.0]).all() and bool((gr != 7.0).any()) and bool((sqr >= 0).all())
    assert torch.equal(g, gr), float((g - gr).abs().max())
    assert torch.equal(sq, sqr), float((sq - sqr).abs().max())


def test_inline_backward_repeats(case):
    """The premise of the comparisons below: the backward of one forward can be run again and gives the same bits."""
    _same(case, case.backward(overlap=0))
    assert case.forks == 0


def test_overlapped_equals_inline(case):
    _same(case, case.backward(overlap=1))
    assert case.forks == case.L  # every layer went to the side stream: the path that was meant is the path that ran


def test_side_stream_held_back(case):
    """300 us in front of every side-stream submission: the chain runs ahead of the weight gradients (a copy overwritten too early,
    a join that does not wait, would show)."""
    _same(case, case.backward(overlap=1, side_us=300.0))
    assert case.forks == case.L


def test_caller_stream_held_back(case):
    """300 us at the start of every layer on the caller's stream: the side stream is as early as its waits allow."""
    _same(case, case.backward(overlap=1, main_us=300.0))
    assert case.forks == case.L


def test_two_backwards_back_to_back(case):
    _same(case, case.backward(overlap=1, twice=True))
    assert case.forks == 2 * case.L


def test_profiled_backward_runs_in_line(case):
    """While vbx_prof_enable(1) is on the weight gradients stay on the caller's stream and the stage table keeps its row."""
    lib = case.lib
    lib.vbx_prof_collect.argtypes = [C.POINTER(ProfEntry), C.c_int]
    lib.vbx_prof_collect.restype = C.c_int
    torch.cuda.synchronize()
    lib.vbx_prof_enable(1)
    try:
        got = case.backward(overlap=1)
        tab = (ProfEntry * 32)()
        n = lib.vbx_prof_collect(tab, 32)
    finally:
        lib.vbx_prof_enable(0)
    assert case.forks == 0
    rows = {e.label.decode(): e.calls for e in tab[:n]}
    assert rows.get("wgrad (4 GEMMs)") == case.L, rows
    _same(case, got)


def test_backward_with_a_stage_reader_runs_in_line(case):
    """on_stage given (a per-stage gradient exchange): every stage's range is final on the caller's stream when its callback fires,
    even with the side stream held back -- nothing was sent there."""
    seen = {}

    def cb(i, rng):
        seen[i] = (rng, case.ts.gflat[rng[0]:rng[1]].clone())

    g, _ = case.backward(overlap=1, side_us=300.0, on_stage=cb)
    assert case.forks == 0 and len(seen) == case.L + 2
    for i, ((lo, hi), snap) in seen.items():
        assert torch.equal(snap, g[lo:hi]), i
    assert torch.equal(g, case.ref[0])  # per-layer and deferred reductions sum in the same order (test_dp_gpu.py)
