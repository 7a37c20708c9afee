"""ODE samplers on the device: midpoint, euler, rk4 and adaptive dopri5, replayed under hipGraph.

Replaces torchdiffeq.odeint(fn, y0, t, method=...) (call site voicebox_pytorch.py:1295; torchdiffeq is third-party, restated in
oracle/ref_loader.py and tests/ode_ref.py -- parity with the library UNPINNED).  Only the final state is kept (the reference stacks
the whole trajectory, voicebox_pytorch.py:1295-1296).  Kernels: csrc/ops.hip (axpy, counter), csrc/ode.hip (include/vbx.h "ODE solvers").

    _Sampler             what every method needs: the split decision, the engines and parts, the static buffers, the adaLN table,
                         the input copy-in and ONE function evaluation (_eval: the forward, or the guidance mix of two forwards)
    _FixedGridSampler    t = linspace(0, 1, steps): ONE interval captured in a hipGraph and replayed steps - 1 times, a device counter
                         selecting the row of the device tables, so no host scalar is baked into the graph; the concurrent halves
      MidpointSampler    f0 = fn(t_i, y);  f1 = fn(t_i + dt/2, y + f0*dt/2);  y <- y + dt*f1   (2 forwards + 2 axpys)
      RKSampler          euler / rk4 from a Butcher tableau (FIXED_TABLEAUS)
    Dopri5Sampler        adaptive: one attempt captured, the host reads the step state back after each
    make_sampler         method name -> sampler (model.py's only entry)

The grid values are computed on the host with the same fp32 torch ops the oracle uses (linspace(0,1,64) has 8 distinct fp32 dt values
-- SURVEY 8(c)).  Midpoint is NOT a third tableau: its step y + f * a runs on vbx_axpy_ctr, a fused multiply-add (csrc/ops.hip, default
contraction: v_pk_fma_f32), the tableau methods' vbx_ode_combine is a multiply, then an add (csrc/ode.hip, fp contract(off), as torch
evaluates y0 + dt * f0) -- the tableau form would change the bits of every midpoint sample.

Concurrent halves.  Every kernel of a forward has a ramp, a drain and -- the GEMMs -- a VALU-bound epilogue during which the
matrix pipes idle (tools/native/gemm_trace.cpp); batch elements are independent in every kernel of the path.  So a batch of
B >= 4 (even) is integrated as TWO half-batches on two streams (the default except at dim 512, see _Sampler.__init__), each with its own engine (activation arena; the packed weights
are shared) and its own captured interval graph: one kernel stream fills the other's holes.  The two integrations never meet
before the end, and the second stream starts SPLIT_OFFSET_US late, so that different kernels of the two forwards overlap
(attention beside GEMMs) rather than the same ones.  Measured on the benchmark shape, 16 intervals: one stream 85.7 ms, two
joined branches of one graph 82.5, two free-running graphs 81.7, with the offset 80.1 (tools/sample_concurrent.py,
tools/sample_offset.py); results bit-identical to the single-stream run.  VBX_SAMPLE_SPLIT=1 restores the single stream (A/B).
Without a graph (use_graph=False) the halves run as fork / join branches per interval.

Unequal lengths (masked=True, run(lens=)).  Row b of the padded batch has len_b real frames.  A masked sampler owns three more static
buffers -- amask [B, N] bool (n < len_b), amask_p [B, R + N] uint8 (the same behind R ones: the copy Engine.forward would otherwise
allocate per call, whose address a captured graph must keep) and key_lens [B] int32 = R + len_b -- sliced into the parts like the
rest and refreshed by _load_inputs, which also writes "masked" / 0 into cond_mask / cond past the lengths and zeroes y0 there.  Every
forward of _eval gets the mask (convolutional position embedding, attention) and the key lengths (vbx_attn_fwd_lens: dead key tiles
are not walked); dopri5's error norm leaves the padding out (vbx_ode_norm_lens); the returned state is zeroed past the lengths.  The
rows of padding frames still go through the GEMMs and norms.  An unmasked sampler passes none of this and launches what it always did.

Packed rows (packed=True, run(plan=); sample(lens=, pack=True)).  The ragged batch is ONE batch row of N = Mp rows (sample_pack.py,
include/vbx.h "packed rows"): B = 1, one stream, a packed engine, not masked.  The caller packs y0 / cond / cond_mask / ids before
run() and unpacks the result after it, outside the captured interval; the sampler owns the static tables seg_start / seg_klen /
tile_seg (capacity Mp / 128 segments), which _load_inputs validates on the host (sample_pack.check_tables) and refreshes by copy
together with the engine's packed rotary tables, and every forward of _eval gets them (vbx_convpos_fwd_segs, vbx_attn_fwd_segs).
All rows share the time point, so B = 1 in the adaLN table is exact.  Fixed-grid methods only.
"""
import contextlib
import ctypes as _C
import os

import torch

from . import _lib
from .engine import precise_enabled


ATTN_KEY_LENS = True  # read when a masked sampler is built.  False: the mask alone, every key tile walked (tools/sample_lens_times.py arm B)

SPLIT_OFFSET_US = float(os.environ.get("VBX_SAMPLE_OFFSET_US", "60"))  # start delay of the second (third, ...) half-batch stream; 30 .. 250 us measured equal


def _to_qkv_owns_cus(cfg, B, N):
    """Does the library serve the model's inference to_qkv GEMM of a full batch with the weight-stationary kernel?  Asked of the
    library (vbx_gemm_route: selected path, VBX_GEMM5, shape), not re-derived here; no buffers exist yet, so the pointer fields
    carry an aligned placeholder."""
    d, some = _lib.GemmDesc(), 256
    Np, I = N + cfg["R"], cfg["H"] * 64
    d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.f16 = _lib.VBX_GEMM_NT, _lib.VBX_EPI_QKV, B * Np, 3 * I, cfg["D"], cfg["D"], cfg["D"], 1
    d.Np, d.H, d.qk_scale = Np, cfg["H"], 8.0 if cfg["qk_norm"] else 0.0
    d.A = d.B = d.q16 = d.k16 = d.v16 = d.rot_cos = d.rot_sin = d.q_gamma = d.k_gamma = some
    return _lib.call_value("vbx_gemm_route", d) == _lib.VBX_GEMM_KERNEL_GEMM5


class _Part:
    """One concurrently integrated slice [lo, hi) of the batch: its engine and its views of the sampler's static buffers."""


class _Sampler:
    """What every method shares.  grid = (stage times of the whole grid, host fp32 [intervals * stride], stride) of a method that
    knows its time points up front: self.t_table, and the adaLN projections of all of them are tabulated (self.ada_tab, row
    ada_stride * counter + slot).  grid = None: every forward evaluates its own projections from p.times."""

    def __init__(self, voicebox, B, N, use_graph=True, tokens=0, guided=False, split=None, grid=None, masked=False, packed=False):
        self.vb, self.B, self.N, self.masked, self.packed = voicebox, B, N, bool(masked), bool(packed)
        if self.packed:  # one batch row of N = Mp packed rows on one stream; the segment tables say which rows are live
            assert B == 1 and N % 128 == 0 and not masked, (B, N, masked)
            split = 1
        if split is None:
            # Default: two concurrent half batches -- EXCEPT where the weight-stationary kernel serves to_qkv / FeedForward-in (dim 512,
            # csrc/gemm5.hip): it owns whole CUs, the half batches' launches cannot interleave with it, and ONE stream is then both
            # faster and deterministic (round 6, ten runs each on one box: 286.0 ms every run against 284-294, mostly 292; with the tiled
            # kernels 317.5 against 298-303 -- the split was a remedy for THEIR idle phases).  VBX_SAMPLE_SPLIT=1 / 2 overrides.
            env = os.environ.get("VBX_SAMPLE_SPLIT")
            if env is None:
                env = "1" if not precise_enabled() and _to_qkv_owns_cus(voicebox._cfg, B, N) else "2"  # (the precise forward has its own GEMMs)
            if env not in ("1", "2"):
                raise ValueError(f"VBX_SAMPLE_SPLIT must be 1 or 2 (concurrent half batches are the only measured, tested split), got {env!r}")
            split = int(env)
        if split not in (1, 2):
            raise ValueError(f"{type(self).__name__}(split={split}): only 1 (one stream) and 2 (two concurrent half batches) are supported")
        if B < 4 or B % split:
            split = 1
        self.split = split
        Bp = B // split
        engines = [voicebox.engine(Bp, N, training=False, packed=self.packed)]
        for i in range(1, split):
            engines.append(voicebox.engine(Bp, N, training=False, slot=i, wpack_from=engines[0]))
        self.eng = engines[0]
        self.flat_gen = self.eng.fp.flat_gen  # the captured graph bakes in addresses inside this flat parameter buffer
        dev = self.eng.device
        D = voicebox._cfg.get("Lc") or voicebox._cfg.get("Din") or voicebox._cfg["D"]  # the ODE state lives in data space (latent_dim / dim_in)
        self.y = torch.zeros(B, N, D, device=dev)
        self.ymid = torch.zeros(B, N, D, device=dev)
        self.f = torch.zeros(B, N, D, device=dev)
        self.cond = torch.zeros(B, N, D, device=dev)
        self.cmask = torch.ones(B, N, dtype=torch.bool, device=dev)
        self.times = torch.zeros(B, device=dev)
        if self.masked:
            R = voicebox._cfg["R"]
            self.amask = torch.ones(B, N, dtype=torch.bool, device=dev)
            self.amask_p = torch.ones(B, R + N, dtype=torch.uint8, device=dev)
            self.lens = torch.full((B,), N, dtype=torch.int32, device=dev)
            self.key_lens = torch.full((B,), R + N, dtype=torch.int32, device=dev) if ATTN_KEY_LENS else None
            self.frames = torch.arange(N, device=dev)[None]
        if self.packed:  # static device tables of include/vbx.h "packed rows", refreshed per call; capacity N / 128 segments
            self.seg_start = torch.zeros(N // 128, dtype=torch.int32, device=dev)
            self.seg_klen = torch.ones(N // 128, dtype=torch.int32, device=dev)
            self.tile_seg = torch.full((N // 128,), -1, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(split, dtype=torch.int32, device=dev)  # one per part (each branch advances its own)
        # text-conditioned models: static token ids; classifier-free guidance (forward_with_cond_scale, :972-985) runs a
        # second, fully dropped evaluation (cond -> null_cond, ids -> null_cond_id) and mixes null + (logits - null) * scale
        self.tokens, self.guided = int(tokens), bool(guided)
        if self.tokens:
            self.ids = torch.zeros(B, self.tokens, dtype=torch.int64, device=dev)
            self.drop_all = torch.ones(B, dtype=torch.uint8, device=dev)
        if self.guided:
            assert self.tokens, "guidance needs a text-conditioned model"
            self.f_null = torch.zeros(B, N, D, device=dev)
            self.f_diff = torch.zeros(B, N, D, device=dev)
            self.g_table = torch.tensor([-1.0, 1.0], device=dev)  # [-1, cond_scale]
        self.parts = []
        for i, eng in enumerate(engines):
            p = _Part()
            p.eng, p.B = eng, Bp
            p.sl = sl = slice(i * Bp, (i + 1) * Bp)
            p.y, p.ymid, p.f, p.cond, p.cmask, p.times = self.y[sl], self.ymid[sl], self.f[sl], self.cond[sl], self.cmask[sl], self.times[sl]
            p.counter = self.counters[i:i + 1]
            if self.masked:
                p.mask_kw = dict(attn_mask=self.amask[sl], attn_mask_p=self.amask_p[sl],
                                 key_lens=self.key_lens[sl] if self.key_lens is not None else None)
            if self.packed:
                p.mask_kw = dict(segs=(self.seg_start, self.seg_klen, self.tile_seg))
            if self.tokens:
                p.ids, p.drop_all = self.ids[sl], self.drop_all[sl]
            if self.guided:
                p.f_null, p.f_diff = self.f_null[sl], self.f_diff[sl]
            self.parts.append(p)
        # adaLN projections of every time point of the grid, evaluated once per weights version instead of once per function
        # evaluation (a 100 MB weight stream + the time MLP per forward at dim 512 / depth 12): every batch element shares the time.
        # VBX_SAMPLE_ADA_TABLE=0: A/B (per-forward projections, bit-identical results).
        self.t_table, self.ada_stride = (grid[0].to(dev), int(grid[1])) if grid is not None else (None, None)
        self.use_ada_table = grid is not None and os.environ.get("VBX_SAMPLE_ADA_TABLE", "1") != "0"
        self.ada_tab, self.ada_key = None, None
        self.graph = None
        self.use_graph = use_graph

    def _zero_tail(self, x):
        """x [B, N, D] fp32: frames at or past the lengths <- 0"""
        _lib.call("vbx_zero_tail_rows", x, self.lens, self.B, self.N, x.shape[-1], _lib.current_stream())

    def _load_inputs(self, cond, cond_mask, cond_token_ids, cond_scale, lens=None, plan=None):
        # eval semantics of the reference: cond_mask None -> everything masked -> cond is zeroed (:1028-1035)
        assert (lens is not None) == self.masked, "a masked sampler runs with lens, an unmasked one without"
        assert (plan is not None) == self.packed, "a packed sampler runs with its plan (sample_pack.pack_plan), any other without"
        if self.packed:
            # the inputs arrive packed (sample_pack.pack_rows: cond 0, cond_mask "masked", id 0 on register and dead rows); the
            # kernels index by the tables, so they are checked here, on the host, before they reach the device
            from .sample_pack import check_tables

            S = len(plan.lens)
            if plan.Mp != self.N or S > self.seg_start.numel():
                raise ValueError(f"packed sampler of {self.N} rows got a plan of {plan.Mp} rows / {S} segments")
            check_tables(plan.seg_start, plan.seg_klen, plan.tile_seg, self.N, S)
            self.seg_start[:S].copy_(plan.seg_start)
            self.seg_klen[:S].copy_(plan.seg_klen)
            self.tile_seg.copy_(plan.tile_seg)
            self.eng.load_packed_rotary(plan.local_row, plan.N)
        if cond is not None:
            self.cond.copy_(cond)
        if cond_mask is not None:
            self.cmask.copy_(cond_mask.to(self.cmask.device))
        else:
            self.cmask.fill_(True)
        if self.masked:  # lens: host int32 [B], validated by the caller
            R = self.vb._cfg["R"]
            self.lens.copy_(lens, non_blocking=True)
            torch.lt(self.frames, self.lens[:, None], out=self.amask)
            self.amask_p[:, R:] = self.amask
            if self.key_lens is not None:
                torch.add(self.lens, R, out=self.key_lens)
            self.cmask.logical_or_(~self.amask)  # past the length: "masked", and 0 in cond, whatever the caller left there
            self._zero_tail(self.cond)
        if self.tokens:
            self.ids.copy_(cond_token_ids.to(self.ids.device))
        if self.guided:
            self.g_table[1] = float(cond_scale)
        for p in self.parts:
            p.eng.bind_params()  # re-pack weights if they changed since the last call
        if self.use_ada_table and not self.vb._cfg.get("plain_norm"):
            key = self.eng.fp.weights_key()
            if self.ada_tab is None:
                self.ada_tab = self.eng.ada_table(self.t_table)  # allocated once: its address is baked into the captured graphs
                self.ada_key = key
            elif key != self.ada_key:
                self.ada_tab.copy_(self.eng.ada_table(self.t_table))
                self.ada_key = key

    def _eval(self, p, x, out, slot=0):
        """One function evaluation of part p at x into `out`: the forward, or under classifier-free guidance the conditioned and the
        fully dropped forward mixed as null + (logits - null) * scale (forward_with_cond_scale, voicebox_pytorch.py:972-985).  The
        time is row ada_stride * counter + slot of the adaLN table, or without one whatever the caller left in p.times."""
        p.eng.dropout_active = False  # sampling is eval (:1268) whatever mode a later forward of the same shape left on the engine
        ada = (self.ada_tab, p.counter, slot, self.ada_stride) if self.ada_tab is not None else None
        mk = p.mask_kw if (self.masked or self.packed) else {}
        if not self.tokens:
            p.eng.forward(x, p.cond, p.cmask, p.times, pred_out=out, ada=ada, **mk)
            return
        vb = self.vb
        p.eng.forward(x, p.cond, p.cmask, p.times, pred_out=out, text=(p.ids, vb.null_cond_id, None, vb.null_cond), ada=ada, **mk)
        if self.guided:
            st, n = _lib.current_stream, out.numel()
            p.eng.forward(x, p.cond, p.cmask, p.times, pred_out=p.f_null,
                          text=(p.ids, vb.null_cond_id, p.drop_all, vb.null_cond), ada=ada, **mk)
            _lib.call("vbx_axpy_dev", out, p.f_null, self.g_table, 0, p.f_diff, n, st())   # logits - null
            _lib.call("vbx_axpy_dev", p.f_null, p.f_diff, self.g_table, 1, out, n, st())   # null + scale * diff


class _FixedGridSampler(_Sampler):
    """A method on t = linspace(0, 1, steps) with S function evaluations per interval.  tables = (stage times [intervals * S],
    coefficients [intervals * S, ...]), host fp32; the subclass's _interval_part(p) launches one interval of one part, reading row
    S * p.counter + slot of them, and advances the counter."""

    def __init__(self, voicebox, B, N, steps, method, tables, use_graph=True, tokens=0, guided=False, split=None, masked=False,
                 packed=False):
        S = tables[0].numel() // (steps - 1)
        super().__init__(voicebox, B, N, use_graph=use_graph, tokens=tokens, guided=guided, split=split, grid=(tables[0], S),
                         masked=masked, packed=packed)
        self.method, self.steps, self.S = method, steps, S
        dev = self.y.device
        self.c_table = tables[1].to(dev)
        self.side_streams = [torch.cuda.Stream(device=dev) for _ in range(self.split - 1)]
        self.part_streams = [torch.cuda.Stream(device=dev) for _ in range(self.split)] if self.split > 1 else []
        self.nfe = S * (steps - 1) * (2 if self.guided else 1)
        # self.graph: split == 1: one interval; split > 1: a list, one interval graph per part

    def _stage_time(self, p, slot):
        if self.ada_tab is None:  # plain-norm models, VBX_SAMPLE_ADA_TABLE=0: the forward reads p.times
            _lib.call("vbx_ode_stage_time", p.times, p.B, self.t_table, p.counter, self.S, slot, _lib.current_stream())

    def _interval(self):
        # part 0 on the current stream, the others on side streams between a fork and a join: parallel branches under capture
        cur = torch.cuda.current_stream()
        for s in self.side_streams:
            s.wait_stream(cur)
        for p, s in zip(self.parts[1:], self.side_streams):
            with torch.cuda.stream(s):
                self._interval_part(p)
        self._interval_part(self.parts[0])
        for s in self.side_streams:
            cur.wait_stream(s)

    @contextlib.contextmanager
    def _cu_share(self):
        """The weight-stationary to_qkv / FeedForward-in kernel (csrc/gemm5.hip) owns whole CUs: with `split` concurrent parts every
        launch gets 1 / split of the chip (include/vbx.h vbx_gemm5_cu_limit; read at launch, so baked into the captured graphs) --
        the two parts' launches then run side by side instead of one behind the other."""
        if self.split == 1:
            yield
            return
        ncu = torch.cuda.get_device_properties(self.y.device).multi_processor_count
        share = int(os.environ.get("VBX_GEMM5_CUS", "0")) or max(ncu // self.split, 1)  # (VBX_GEMM5_CUS=<n>: A/B of the share)
        _lib.call("vbx_gemm5_cu_limit", share)
        try:
            yield
        finally:
            _lib.call("vbx_gemm5_cu_limit", 0)

    def _capture(self):
        with self._cu_share():
            # warm up on a side stream (one-time kernel attribute calls, weight packing), then capture one interval
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.counters.zero_()
                self._interval()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            if self.split == 1:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._interval()
                self.graph = g
            else:
                self.graph = []
                for p in self.parts:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._interval_part(p)
                    self.graph.append(g)

    def _replay_parts(self):
        """steps-1 intervals of every part: each part's graph on its own stream, the streams never meet before the end."""
        cur = torch.cuda.current_stream()
        for s in self.part_streams:
            s.wait_stream(cur)
        for i, s in enumerate(self.part_streams[1:], 1):
            with torch.cuda.stream(s):
                _lib.call("vbx_stream_delay", SPLIT_OFFSET_US * i, _lib.current_stream())
        for _ in range(self.steps - 1):
            for g, s in zip(self.graph, self.part_streams):
                with torch.cuda.stream(s):
                    g.replay()
        for s in self.part_streams:
            cur.wait_stream(s)

    def run(self, y0, cond=None, cond_mask=None, cond_token_ids=None, cond_scale=1.0, lens=None, plan=None):
        self._load_inputs(cond, cond_mask, cond_token_ids, cond_scale, lens, plan)
        if self.use_graph and self.graph is None:
            self._capture()
        self.y.copy_(y0)
        if self.masked:
            self._zero_tail(self.y)
        self.counters.zero_()
        if self.use_graph and self.split > 1:
            self._replay_parts()
        else:
            for _ in range(self.steps - 1):
                if self.use_graph:
                    self.graph.replay()
                else:
                    with self._cu_share():
                        self._interval()
        out = self.y.clone()
        if self.masked:
            self._zero_tail(out)
        return out

    def stats(self):
        return {"method": self.method, "nfe": self.nfe, "accepted": self.steps - 1, "rejected": 0}


def midpoint_tables(steps):
    """Host fp32 tables of the midpoint rule on t = linspace(0, 1, steps), [2 * intervals] each: times [t0, t0 + dt/2] and
    coefficients [dt/2, dt] per interval."""
    assert steps >= 2, "need at least two time points"
    t = torch.linspace(0, 1, steps)  # host fp32, as the CPU oracle
    t0, dt = t[:-1], t[1:] - t[:-1]
    half = 0.5 * dt
    return (torch.stack((t0, t0 + half), dim=1).reshape(-1).contiguous(),
            torch.stack((half, dt), dim=1).reshape(-1).contiguous())


class MidpointSampler(_FixedGridSampler):
    """torchdiffeq's fixed-grid midpoint.  Its own step on vbx_axpy_ctr (fused y + f * a), not a tableau: see the module docstring."""

    def __init__(self, voicebox, B, N, steps, use_graph=True, tokens=0, guided=False, split=None, masked=False, packed=False):
        super().__init__(voicebox, B, N, steps, "midpoint", midpoint_tables(steps), use_graph=use_graph, tokens=tokens, guided=guided,
                         split=split, masked=masked, packed=packed)

    def _interval_part(self, p):
        st = _lib.current_stream
        n = p.y.numel()
        self._stage_time(p, 0)
        self._eval(p, p.y, p.f, 0)
        _lib.call("vbx_axpy_ctr", p.y, p.f, self.c_table, p.counter, 0, p.ymid, n, st())
        self._stage_time(p, 1)
        self._eval(p, p.ymid, p.f, 1)
        _lib.call("vbx_axpy_ctr", p.y, p.f, self.c_table, p.counter, 1, p.y, n, st())
        _lib.call("vbx_counter_add", p.counter, 1, st())


# Fixed-grid explicit RK tableaus: (c, a, b) -- stage times t0 + c dt (c = 1: t1 itself), stage inputs y0 + dt sum_j a_ij k_j, step
# dy = dt sum_j b_j k_j.  rk4 is torchdiffeq's 3/8 rule (rk4_alt_step_func), not the classic RK4.
FIXED_TABLEAUS = {
    "euler": ((0.0,), (), (1.0,)),
    "rk4": ((0.0, 1 / 3, 2 / 3, 1.0), ((1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125)),
}


def fixed_grid_tables(method, steps):
    """Host fp32 tables of a fixed-grid method on t = linspace(0, 1, steps): stage times [intervals * S] (t0 + dt * c; c = 1 is t1
    itself) and coefficients [intervals * S, S]: per interval, rows 0 .. S-2 the stage inputs' dt * a_ij, row S-1 the step's dt * b_j."""
    c, a, b = FIXED_TABLEAUS[method]
    S = len(b)
    assert steps >= 2, "need at least two time points"
    t = torch.linspace(0, 1, steps)
    t0, t1 = t[:-1], t[1:]
    dt = t1 - t0
    times = [t0 if ci == 0 else (t1 if ci == 1 else t0 + dt * ci) for ci in c]
    rows = []
    for coefs in list(a) + [b]:
        r = torch.zeros(steps - 1, S)
        for j, v in enumerate(coefs):
            r[:, j] = dt * v
        rows.append(r)
    return torch.stack(times, dim=1).reshape(-1).contiguous(), torch.stack(rows, dim=1).reshape(-1, S).contiguous()


def _ptrs(ts):
    return (_C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _floats(vals):
    return (_C.c_float * len(vals))(*vals)


class RKSampler(_FixedGridSampler):
    """torchdiffeq's fixed-grid euler and rk4 (FixedGridODESolver: y1 = y0 + dy per interval).  The stage times and the coefficients
    dt * a_ij, dt * b_j are formed on the host in fp32 torch arithmetic (fixed_grid_tables) and live in device tables
    [intervals * S] / [intervals * S][S] indexed by the part's device counter; the adaLN table holds every STAGE time."""

    def __init__(self, voicebox, B, N, steps, method, use_graph=True, tokens=0, guided=False, split=None, masked=False, packed=False):
        if method not in FIXED_TABLEAUS:
            raise ValueError(f"RKSampler: no fixed-grid tableau {method!r} (have {sorted(FIXED_TABLEAUS)})")
        super().__init__(voicebox, B, N, steps, method, fixed_grid_tables(method, steps), use_graph=use_graph, tokens=tokens,
                         guided=guided, split=split, masked=masked, packed=packed)
        self.ks = [self.f] + [torch.zeros_like(self.y) for _ in range(self.S - 1)]  # stage derivatives; the stage inputs go to ymid
        for p in self.parts:
            p.k = [k[p.sl] for k in self.ks]

    def _interval_part(self, p):
        st = _lib.current_stream
        n = p.y.numel()
        S = self.S
        for s in range(S):
            x = p.y
            if s:
                x = p.ymid
                _lib.call("vbx_ode_combine", x, p.y, _ptrs(p.k[:s]), s, self.c_table, S, p.counter, S, s - 1, n, st())
            self._stage_time(p, s)
            self._eval(p, x, p.k[s], s)
        _lib.call("vbx_ode_combine", p.y, p.y, _ptrs(p.k), S, self.c_table, S, p.counter, S, S - 1, n, st())
        _lib.call("vbx_counter_add", p.counter, 1, st())


def _f32(vals):
    return [float(v) for v in torch.tensor(vals, dtype=torch.float64).float()]


# torchdiffeq's Dormand-Prince-Shampine tableau (rk_common / dopri5), as the solver holds it: cast to the state's dtype (fp32)
DP_ALPHA = _f32([1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0])
DP_BETA = [_f32(r) for r in ([1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9],
                             [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
                             [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
                             [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84])]
DP_C_ERROR = _f32([35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
                   11 / 84 - 649 / 6300, -1. / 60.])
DP_C_MID = _f32([6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
                 187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2])

# include/vbx.h: the dopri5 step state record and the ODE kernel modes
(DP_T, DP_DT, DP_T0, DP_T1, DP_DT32, DP_RATIO, DP_H0, DP_D1, DP_NFE, DP_ACCEPTED, DP_REJECTED, DP_LAST, DP_DONE, DP_BAD, DP_ATOL,
 DP_RTOL, DP_TEND) = range(17)
DP_STATE = 20
TIME_STAGE, TIME_END, TIME_PROBE = 1, 2, 3
NORM_ERROR, NORM_INIT0, NORM_INIT1 = 0, 1, 2


class Dopri5Sampler(_Sampler):
    """torchdiffeq's adaptive dopri5 (RKAdaptiveStepsizeODESolver with the Dormand-Prince-Shampine tableau, FSAL, order 5), t from 0
    to 1 with tolerances atol / rtol.  The RMS error norm couples the whole batch: ONE stream (split 1).  The stage times are not
    known in advance, so there is no grid and every forward evaluates its own adaLN projections (no table).  The initial step (f0,
    the probe, h) runs eagerly; one attempt -- 6 forwards, the stage combinations, the two-launch error norm with the controller
    and the commit -- is captured as a graph (the first attempt runs eagerly and warms up every kernel).  The host replays it and
    reads the 160-byte step state back after each attempt (one small synchronisation per 6 function evaluations) until t >= 1, then
    evaluates the dense-output quartic of the last accepted step at t = 1 (steps are not clipped: the last one overshoots).
    `steps` does not change the result (only the final time point is returned) and is not kept; with no grid, t_table and
    ada_stride are None and _eval passes ada=None."""

    def __init__(self, voicebox, B, N, steps, use_graph=True, tokens=0, guided=False, atol=1e-5, rtol=1e-5, max_attempts=10000,
                 masked=False):
        super().__init__(voicebox, B, N, use_graph=use_graph, tokens=tokens, guided=guided, split=1, grid=None, masked=masked)
        self.atol, self.rtol, self.max_attempts = float(atol), float(rtol), int(max_attempts)
        dev = self.y.device
        self.ks = [self.f] + [torch.zeros_like(self.y) for _ in range(6)]  # k1 .. k7
        self.y1 = torch.zeros_like(self.y)
        self.out = torch.zeros_like(self.y)
        self.state = torch.zeros(DP_STATE, dtype=torch.float64, device=dev)
        self.slab = torch.zeros(_lib.lib().vbx_ode_norm_slab_doubles(self.y.numel()), dtype=torch.float64, device=dev)
        self.mult = 2 if self.guided else 1
        self.last_stats = self.nfe = None  # counted on the device: known after a run

    def _norm(self, mode, y1, ks, c, S):
        """the RMS norm + controller over the whole state, or under lens over the real frames only"""
        n, st = self.y.numel(), _lib.current_stream()
        if self.masked:
            _lib.call("vbx_ode_norm_lens", self.state, self.slab, mode, self.y, y1, _ptrs(ks), c, S, n, self.mult, self.lens, self.B,
                      self.y.shape[-1], st)
        else:
            _lib.call("vbx_ode_norm", self.state, self.slab, mode, self.y, y1, _ptrs(ks), c, S, n, self.mult, st)

    def _attempt(self):
        p, st, n = self.parts[0], _lib.current_stream, self.y.numel()
        for i in range(6):
            x = self.y1 if i == 5 else self.ymid  # the last stage input is the 5th-order solution y1 (c_sol == beta[-1])
            _lib.call("vbx_ode_combine_dp", x, self.y, _ptrs(self.ks[:i + 1]), _floats(DP_BETA[i]), i + 1, self.state, DP_DT, n, st())
            mode = TIME_END if DP_ALPHA[i] == 1.0 else TIME_STAGE
            _lib.call("vbx_ode_stage_time_dp", p.times, self.B, self.state, DP_ALPHA[i], mode, st())
            self._eval(p, x, self.ks[i + 1])
        self._norm(NORM_ERROR, self.y1, self.ks, _floats(DP_C_ERROR), 7)
        _lib.call("vbx_ode_commit", self.y, self.ks[0], self.y1, self.ks[6], self.state, n, st())

    def _initial(self):
        """_select_initial_step: f0 = f(0, y0), d0 / d1, the probe f1 = f(h0, y0 + h0 f0), d2 -> the first dt."""
        p, st, n = self.parts[0], _lib.current_stream, self.y.numel()
        init = torch.zeros(DP_STATE, dtype=torch.float64)
        init[DP_T], init[DP_TEND], init[DP_ATOL], init[DP_RTOL] = 0.0, 1.0, self.atol, self.rtol
        self.state.copy_(init)
        p.times.fill_(0.0)
        self._eval(p, self.y, self.ks[0])
        self._norm(NORM_INIT0, None, self.ks[:1], None, 1)
        _lib.call("vbx_ode_combine_dp", self.ymid, self.y, _ptrs(self.ks[:1]), _floats([1.0]), 1, self.state, DP_H0, n, st())
        _lib.call("vbx_ode_stage_time_dp", p.times, self.B, self.state, 0.0, TIME_PROBE, st())
        self._eval(p, self.ymid, self.ks[1])
        self._norm(NORM_INIT1, None, self.ks[:2], None, 2)

    def _capture(self):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._attempt()
        self.graph = g

    def run(self, y0, cond=None, cond_mask=None, cond_token_ids=None, cond_scale=1.0, lens=None):
        self._load_inputs(cond, cond_mask, cond_token_ids, cond_scale, lens)
        self.y.copy_(y0)
        if self.masked:
            self._zero_tail(self.y)
        self._initial()
        attempts = 0
        while True:
            if attempts:
                s = self.state.tolist()  # the one synchronisation per attempt
                if s[DP_BAD]:
                    what = "non-finite values in the state or its error estimate" if s[DP_BAD] == 1 else "underflow in dt"
                    raise RuntimeError(f"dopri5: {what} at t = {s[DP_T]!r} (dt {s[DP_DT]!r}, error ratio {s[DP_RATIO]!r})")
                if s[DP_DONE]:
                    break
                if attempts >= self.max_attempts:
                    raise RuntimeError(f"dopri5: {attempts} attempts (max_attempts) without reaching t = 1: t = {s[DP_T]!r}, "
                                       f"dt = {s[DP_DT]!r}")
            if self.use_graph and attempts:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
            else:
                self._attempt()
            attempts += 1
        _lib.call("vbx_ode_dense", self.out, self.y, self.y1, _ptrs(self.ks), _floats(DP_C_MID), self.state, self.y.numel(),
                  _lib.current_stream())
        self.last_stats = {"method": "dopri5", "nfe": int(s[DP_NFE]), "accepted": int(s[DP_ACCEPTED]), "rejected": int(s[DP_REJECTED])}
        self.nfe = self.last_stats["nfe"]
        out = self.out.clone()
        if self.masked:
            self._zero_tail(out)
        return out

    def stats(self):
        return dict(self.last_stats)


def make_sampler(method, voicebox, B, N, steps, *, use_graph=True, tokens=0, guided=False, atol=1e-5, rtol=1e-5, masked=False,
                 packed=False):
    """The sampler of a torchdiffeq method name (atol / rtol: read by dopri5 only; masked: it runs with lens; packed: it runs one
    batch row of N = Mp packed rows with a plan, fixed-grid methods only)."""
    kw = dict(use_graph=use_graph, tokens=tokens, guided=guided, masked=masked)
    if packed:
        if method == "dopri5":
            raise NotImplementedError("dopri5 does not serve pack=True: its error norm would have to leave the dead rows out and "
                                      "vbx_ode_norm_lens is laid out for [B, N] -- use euler, midpoint or rk4, or lens= without pack")
        kw["packed"] = True
    if method == "midpoint":
        return MidpointSampler(voicebox, B, N, steps, **kw)
    if method == "dopri5":
        return Dopri5Sampler(voicebox, B, N, steps, atol=atol, rtol=rtol, **kw)
    return RKSampler(voicebox, B, N, steps, method, **kw)  # ValueError for a name without a tableau
