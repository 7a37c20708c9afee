"""Data-parallel CFM training step: one process per GPU, replicated weights, batch sharded across ranks,
flat fp32 gradient buffer all-reduced over RCCL/xGMI in stage-sized buckets while the backward of earlier
layers is still running, then global-norm clip + fused Adam on the flat buffers.

Semantics to match (VoiceBoxTrainer.train_step, trainer.py:237-313): each rank's loss is
the mean over its local batch; gradients are averaged over ranks (DDP), clipped to max_grad_norm = 0.5
(trainer.py:274-275), then Adam(lr, betas=(0.9, 0.99)) (optimizer.py:10-35, wd = 0 default trainer.py:74).
"""
import os

import torch
import torch.distributed as dist

from . import _lib
from .masks import take_draw


def force_dist():
    return os.environ.get("VBX_FORCE_DIST") == "1"


class GradBucketReducer:
    """All-reduce(sum) of a flat gradient buffer in contiguous buckets as backward stages complete.
    Device-agnostic (gloo on CPU in tests, RCCL on GPUs).  xGMI is point-to-point (ring all-reduce is per-link
    bound) so buckets are large: whole backward stages are merged until `bucket_bytes` is reached."""

    def __init__(self, gflat, stage_ranges, group=None, bucket_bytes=64 << 20, comm_stream=None, comm_dtype=None, tail_bytes=16 << 20,
                 stage_buf=None, shard=False, skip_ranges=()):
        """shard=True: every bucket is REDUCE-SCATTERED instead of all-reduced -- rank r ends up with the sum of chunk r (1 / world
        of the bucket, in place) and `owned` lists the flat ranges this rank must clip / Adam before all-gathering the updated
        parameters (TrainStep(grad_mode="shard")): the optimizer's HBM traffic and arithmetic drop by the world size; the wire
        carries the same bytes as a ring all-reduce (whose two halves these are)."""
        self.g, self.ranges, self.group, self.bucket_bytes = gflat, stage_ranges, group, bucket_bytes
        # skip_ranges: flat ranges that are NOT exchanged here -- the adaLN projection weight blocks whose gradient travels in factor
        # form (TrainStep(adaln_grads="factors"): all-gather of dada / temb, < 1 MB per rank, instead of 201 MB of products).  A stage
        # that contains one is exchanged as the pieces around it.  Known cost: a skipped block ends the pending run, so with
        # factor exchange the buckets are per-layer pieces (~17 MB at dim 512, one or two collectives per layer) and `bucket_bytes` only
        # caps them; merging across skipped blocks needs the adaLN blocks laid out apart from the layer weights (or a gather through the
        # staging buffer) and was left out -- the pieces still overlap the backward of the earlier layers.
        self.skip_ranges = sorted((int(a), int(b)) for a, b in skip_ranges)
        self.wire_floats = 0  # floats handed to collectives by this reducer (bench.py reports the wire bytes per step)
        self.shard = bool(shard)
        self.owned = []
        # The LAST bucket cannot overlap any backward work (nothing is left to run), so it must be small: as soon as what remains
        # to be produced fits `tail_bytes`, the pending stages are flushed instead of being merged with the tail.  With the model's
        # stage order (head, layer L-1 .. 0, embed + time MLP) only the embed stage (a few MB) is exchanged un-overlapped; before,
        # layers 1-0 + embed (~70 MB at dim 512) formed the final bucket.
        self.tail_bytes = tail_bytes
        self.total_hi = max((hi for _, hi in stage_ranges), default=gflat.numel()) if stage_ranges else gflat.numel()
        self.stage_buf = stage_buf  # persistent wire-dtype staging buffer (same numel as gflat); allocated on demand otherwise
        # optional gradient compression on the wire (DDP's bf16_compress_hook): halves the 4 B/param exchange; off by default
        self.comm_dtype = comm_dtype if comm_dtype not in (None, torch.float32) else None
        self.staged = []
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # VBX_FORCE_DIST=1: issue the collectives even at world size 1 (exercises the RCCL path -- comm stream, async work,
        # record_stream -- on a single GPU; an all-reduce over one rank is the identity)
        self.active = self.world > 1 or (force_dist() and dist.is_available() and dist.is_initialized())
        self.rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
        # Which collectives the shard mode uses is decided HERE, per reducer, from the backend and the device of the buffer (ADVICE r4:
        # a try / except fallback flipped a process-global flag on any RuntimeError -- a real RCCL error was hidden, and a failure on
        # one rank made the ranks issue different collectives).  RCCL (backend "nccl") has in-place reduce_scatter_tensor /
        # all_gather_into_tensor on device tensors; gloo gets the all-reduce / per-chunk broadcast forms.  Errors propagate.
        self.native_shard_collectives = bool(self.active and gflat.is_cuda and dist.get_backend(group) == "nccl")
        self.uneven_logged = False
        self.comm_stream = comm_stream
        self.pending_lo = None
        self.pending_hi = None
        self.works = []
        self.buckets_launched = []

    def chunk_of(self, lo, hi, r=None):
        """Rank r's chunk of bucket [lo, hi): equal parts.  Flat slots and stage boundaries are multiples of 64 floats, so a bucket
        divides evenly by every POWER-OF-TWO world size up to 64; for other world sizes (3, 6, 7 ...) the remainder goes to the last
        rank and the exchange falls back to all-reduce + per-chunk broadcasts (no traffic saved; logged once)."""
        r = self.rank if r is None else r
        n = (hi - lo) // self.world
        return lo + r * n, (hi if r == self.world - 1 else lo + (r + 1) * n)

    def _collective(self, view, lo, hi):
        if not self.shard:
            return dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        n = (hi - lo) // self.world
        if n * self.world != hi - lo:  # world size not a power of two: all-reduce, every rank keeps its chunk
            if not self.uneven_logged and self.rank == 0:
                print(f"voicebox_pytorch_amd.dp: bucket of {hi - lo} floats does not divide by world size {self.world}: "
                      "shard mode exchanges it by all-reduce + broadcasts (no wire traffic saved)", flush=True)
            self.uneven_logged = True
            return dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        if self.native_shard_collectives:  # in place: the output is this rank's slice of the input
            self.used_reduce_scatter = True
            return dist.reduce_scatter_tensor(view[self.rank * n:(self.rank + 1) * n], view, op=dist.ReduceOp.SUM, group=self.group,
                                              async_op=True)
        return dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    used_reduce_scatter = False  # set on the instance when the in-place reduce-scatter path ran (asserted by the RCCL test)

    def _launch(self, lo, hi):
        if hi <= lo:
            return
        self.buckets_launched.append((lo, hi))
        self.wire_floats += hi - lo
        if self.shard:
            self.owned.append(self.chunk_of(lo, hi))
        if not self.active:
            return
        view = self.g[lo:hi]
        if self.comm_stream is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                if self.comm_dtype is not None:
                    view = self._stage(lo, hi)
                self.works.append(self._collective(view, lo, hi))
        else:
            if self.comm_dtype is not None:
                view = self._stage(lo, hi)
            self.works.append(self._collective(view, lo, hi))

    def _stage(self, lo, hi):
        if self.stage_buf is None or self.stage_buf.dtype != self.comm_dtype or self.stage_buf.numel() < self.g.numel():
            self.stage_buf = torch.empty(self.g.numel(), dtype=self.comm_dtype, device=self.g.device)  # once, not per bucket per step
        buf = self.stage_buf[lo:hi]
        buf.copy_(self.g[lo:hi])
        self.staged.append((lo, hi, buf))
        return buf

    def stage_done(self, i, rng=None):
        lo, hi = rng if rng is not None else self.ranges[i]
        if self.skip_ranges:
            pieces, cur = [], lo
            for a, b in self.skip_ranges:
                if b <= lo or a >= hi:
                    continue
                if a > cur:
                    pieces.append((cur, a))
                cur = max(cur, b)
            if cur < hi:
                pieces.append((cur, hi))
            for plo, phi in pieces:
                self._piece_done(plo, phi)
            return
        self._piece_done(lo, hi)

    def _piece_done(self, lo, hi):
        if self.pending_lo is not None and lo != self.pending_hi and self.skip_ranges:
            self._launch(self.pending_lo, self.pending_hi)  # a skipped block lies in between: the pending run ends here
            self.pending_lo = None
        if self.pending_lo is None:
            self.pending_lo, self.pending_hi = lo, hi
        else:
            assert lo == self.pending_hi, "stages must complete in flat-buffer order"
            self.pending_hi = hi
        es = self.g.element_size()
        remaining = (self.total_hi - self.pending_hi) * es  # gradients still to be produced by later stages
        pending = (self.pending_hi - self.pending_lo) * es
        # (a small pending range is simply merged with the tail: the final bucket then stays <= 2 * tail_bytes)
        if pending >= self.bucket_bytes or (0 < remaining <= self.tail_bytes < pending):
            self._launch(self.pending_lo, self.pending_hi)
            self.pending_lo = None

    def finish(self):
        if self.pending_lo is not None:
            self._launch(self.pending_lo, self.pending_hi)
            self.pending_lo = None
        for w in self.works:
            w.wait()  # makes the current stream wait for the collective
        self.works = []
        for lo, hi, buf in self.staged:  # decompress the reduced buckets back into the fp32 gradient buffer
            if self.shard and self.active:  # only this rank's chunk holds the sum
                clo, chi = self.chunk_of(lo, hi)
                self.g[clo:chi].copy_(buf[clo - lo:chi - lo])
            else:
                self.g[lo:hi].copy_(buf)   # (the staging buffer is persistent and owned by the caller: no record_stream needed)
        self.staged = []

    def all_gather(self, flat):
        """shard mode, after the owners updated their chunks of `flat` (the parameters): every bucket's chunks are all-gathered in
        place (rank r's input is its own slice of the output), issued on the CURRENT stream and waited for before returning."""
        if not (self.shard and self.active):
            return
        works = []
        for lo, hi in self.buckets_launched:
            n = (hi - lo) // self.world
            view = flat[lo:hi]
            if n * self.world != hi - lo:
                for r in range(self.world):  # uneven (never with this layout): broadcast every chunk from its owner
                    clo, chi = self.chunk_of(lo, hi, r)
                    works.append(dist.broadcast(flat[clo:chi], src=dist.get_global_rank(self.group, r) if self.group is not None else r,
                                                group=self.group, async_op=True))
                continue
            if self.native_shard_collectives:
                works.append(dist.all_gather_into_tensor(view, view[self.rank * n:(self.rank + 1) * n], group=self.group, async_op=True))
                continue
            for r in range(self.world):
                works.append(dist.broadcast(view[r * n:(r + 1) * n], src=dist.get_global_rank(self.group, r) if self.group is not None else r,
                                            group=self.group, async_op=True))
        for w in works:
            w.wait()


def gather_adaln_factors(dada, temb, group=None):
    """Every rank's adaLN gradient factors -> (dada_all [L, W * B, J4], temb_all [W * B, Th], floats this rank put on the wire).
    dada [L, B, J4], temb [B, Th] (fp32, any device the backend serves).  The gradient of layer l's adaLN weight block summed over the
    ranks is dada_all[l]^T . temb_all -- what an all-reduce of the per-rank products dada_r[l]^T . temb_r would deliver, from
    B * (L * J4 + Th) floats per rank instead of L * J4 * Th.
    REQUIRES the same local batch B on every rank (an equal-size all-gather; what a DistributedSampler / Accelerate's even batches give):
    a caller that shards unevenly must use the materialised exchange (`adaln_exchange="materialize"`), whose all-reduce does not depend
    on B -- with unequal B this collective errors or hangs (README "Known limits")."""
    L, B, J4 = dada.shape
    Th = temb.shape[1]
    mine = torch.cat((dada.reshape(-1), temb.reshape(-1)))
    W = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    if W > 1:
        allf = torch.empty(W * mine.numel(), dtype=mine.dtype, device=mine.device)
        if mine.is_cuda and dist.get_backend(group) == "nccl":
            dist.all_gather_into_tensor(allf, mine, group=group)
        else:
            dist.all_gather(list(allf.view(W, -1).unbind(0)), mine, group=group)
        allf = allf.view(W, -1)
    else:
        allf = mine.view(1, -1)
    dada_all = allf[:, :L * B * J4].reshape(W, L, B, J4).permute(1, 0, 2, 3).reshape(L, W * B, J4).contiguous()
    temb_all = allf[:, L * B * J4:].reshape(W * B, Th).contiguous()
    return dada_all, temb_all, int(mine.numel())


class WarmupCosineLR:
    """The learning-rate rule of VoiceBoxTrainer.train_step (trainer.py:231-253, scheduler built at :144-145): linear warm-up
    `initial_lr + (lr - initial_lr) * step / num_warmup_steps` while `step < num_warmup_steps`, afterwards one
    `CosineAnnealingLR(T_max=num_train_steps, eta_min=0).step()` per training step -- torch's *recursive* update applied to
    whatever rate the warm-up left in the optimizer, which is what this class replays on the host (pure Python floats)."""

    def __init__(self, lr, num_train_steps, num_warmup_steps=0, initial_lr=1e-5):
        import math

        self._math = math
        self.lr, self.initial_lr = float(lr), float(initial_lr)
        self.T, self.warm = int(num_train_steps), int(num_warmup_steps or 0)
        self.cur = float(lr)   # the optimizer's param_group['lr']
        self.sched_epoch = 0   # CosineAnnealingLR.last_epoch

    def rate_for_step(self, step):
        """Call once per training step with the 0-based step counter; returns the rate that step must use."""
        m = self._math
        if step < self.warm:
            self.cur = self.initial_lr + (self.lr - self.initial_lr) * step / self.warm
        else:
            self.sched_epoch += 1
            t, T = self.sched_epoch, self.T
            if (t - 1 - T) % (2 * T) == 0:   # torch.optim.lr_scheduler.CosineAnnealingLR.get_lr, eta_min = 0
                self.cur = self.cur + self.lr * (1 - m.cos(m.pi / T)) / 2
            else:
                self.cur = (1 + m.cos(m.pi * t / T)) / (1 + m.cos(m.pi * (t - 1) / T)) * self.cur
        return self.cur


def trainable_ranges(fp, flags, exclude=()):
    """Flat ranges [lo, hi) of the slots of `fp.order` whose flag is set, minus the `exclude` ranges: hi rounded up to 4 floats (the
    padding behind a slot is never written: zeros in every gradient buffer), neighbours merged across that padding.  What the clip
    norm of a partly frozen model is taken over (vbx_sumsq_ranges reads 16-byte groups)."""
    out = []
    excl = sorted(exclude)
    for s, on in zip(fp.order, flags):
        if not on:
            continue
        lo = fp.offsets[s]
        hi = lo + (fp.slots[s].numel() + 3) // 4 * 4
        if any(a <= lo and hi <= b for a, b in excl):
            continue
        nxt = (hi + 63) // 64 * 64
        if out and out[-1][2] == lo:
            out[-1][1], out[-1][2] = hi, nxt
        else:
            out.append([lo, hi, nxt])
    return [(lo, hi) for lo, hi, _ in out]


def range_chunks(ranges, limit=64):
    """vbx_sumsq_ranges takes at most 64 ranges per launch: the list in launches of `limit`."""
    return [ranges[i:i + limit] for i in range(0, len(ranges), limit)]


def filter_adam_segments(segs, frozen):
    """The vbx_adam_seg table of a partly frozen model.  segs: dicts with the fields of vbx_adam_seg (off, count, dst_bf16, dst_f16,
    dst_f32, cols, dst_ld, rowmap, F) tiling the flat buffer; frozen: [lo, hi) slot ranges that must not be touched.  A segment
    inside a frozen range is dropped (the table supports gaps: that is how the factor-form adaLN blocks are left out), one that
    straddles is split.  A packed segment ([rows, cols] written to its operand copy) is cut at whole rows only -- the adaLN weight
    block (four tensors of D rows each) and the one-row adaLN bias block are the packed segments that hold more than one tensor --
    and the pieces' destinations move with them.  block0 is renumbered; returns (segments, total_blocks)."""
    out = []
    frozen = sorted(frozen)
    for sg in segs:
        lo, hi = sg["off"], sg["off"] + sg["count"]
        keep, cur = [], lo
        for a, b in frozen:
            if b <= cur or a >= hi:
                continue
            if a > cur:
                keep.append((cur, a))
            cur = max(cur, b)
        if cur < hi:
            keep.append((cur, hi))
        packed = bool(sg["dst_bf16"] or sg["dst_f16"] or sg["dst_f32"])
        for a, b in keep:
            if (a, b) == (lo, hi):
                out.append(dict(sg))
                continue
            piece = dict(sg, off=a, count=b - a)
            if packed:
                cols, rows = sg["cols"], sg["count"] // sg["cols"]
                if rows == 1:  # one row (the adaLN bias block): any cut, the piece is a shorter row further right
                    shift, piece["cols"] = a - lo, b - a
                else:
                    assert sg["rowmap"] == 0 and (a - lo) % cols == 0 and (b - lo) % cols == 0, "a packed segment splits at whole rows only"
                    shift = (a - lo) // cols * sg["dst_ld"]
                for k, width in (("dst_bf16", 2), ("dst_f16", 2), ("dst_f32", 4)):
                    if sg[k]:
                        piece[k] = sg[k] + shift * width
            out.append(piece)
    blocks = 0
    for sg in out:
        sg["block0"] = blocks
        blocks += 0 if sg["rowmap"] == 2 else (sg["count"] + 2047) // 2048
    return out, blocks


def ema_decay_at(t, ema_decay, ema_update_after_step=0, ema_inv_gamma=1.0, ema_power=None):
    """The decay TrainStep(ema_decay=) uses at optimizer step t (1-based: TrainStep.steps after its increment); pure host arithmetic in
    Python floats (the C ABI receives the value converted to fp32).  t <= ema_update_after_step: 0.0 (the average is a copy of the
    weights); otherwise, with k = t - ema_update_after_step, `ema_decay` (ema_power=None) or the warm-up
    min(ema_decay, 1 - (1 + k / ema_inv_gamma) ** -ema_power).  The keywords follow ema-pytorch's; parity with that library is not
    pinned by any test (it is not a dependency)."""
    t, after = int(t), int(ema_update_after_step)
    if t <= after:
        return 0.0
    if ema_power is None:
        return float(ema_decay)
    k = t - after
    return min(float(ema_decay), 1.0 - (1.0 + k / float(ema_inv_gamma)) ** -float(ema_power))


def check_ema_hyper(ema_decay, ema_update_after_step=0, ema_inv_gamma=1.0, ema_power=None):
    """ValueError for hyper-parameters outside the contract (before anything is allocated)."""
    if ema_decay is None:
        return
    if not (isinstance(ema_decay, (int, float)) and 0.0 <= float(ema_decay) < 1.0):
        raise ValueError(f"ema_decay must be in [0, 1) (got {ema_decay!r})")
    if ema_power is not None and not (isinstance(ema_power, (int, float)) and float(ema_power) > 0.0):
        raise ValueError(f"ema_power must be > 0 (got {ema_power!r})")
    if not (isinstance(ema_inv_gamma, (int, float)) and float(ema_inv_gamma) > 0.0):
        raise ValueError(f"ema_inv_gamma must be > 0 (got {ema_inv_gamma!r})")
    if not (isinstance(ema_update_after_step, int) and ema_update_after_step >= 0):
        raise ValueError(f"ema_update_after_step must be an integer >= 0 (got {ema_update_after_step!r})")


def adaln_rule(flags_by_slot, depth):
    """What a partly frozen model does with the adaLN weight gradients: "all" (every G1W / B1W / G2W / B2W trainable: the factor path
    as it is), "none" (all frozen: no factor Adam and no Gram terms; the backward may still leave the blocks unwritten) or "mixed"
    (fall back to the materialised gradient)."""
    fl = [flags_by_slot[f"L{l}.{n}"] for l in range(depth) for n in ("G1W", "B1W", "G2W", "B2W") if f"L{l}.{n}" in flags_by_slot]
    if not fl or all(fl):
        return "all"
    return "none" if not any(fl) else "mixed"


class TrainStep:
    def __init__(self, wrapper, lr=3e-4, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=0.5, group=None,
                 bucket_bytes=64 << 20, broadcast_params=True, lr_schedule=None, grad_comm_dtype=None, wd=0., length_bucket=0,
                 grad_mode="allreduce", adaln_grads="auto", ema_decay=None, ema_update_after_step=0, ema_inv_gamma=1.0, ema_power=None):
        """adaln_grads: what step() does with the gradient of the adaLN projection WEIGHTS (voicebox_pytorch.py:256-276; 49 % of the
        parameters at dim 512 / depth 12, each layer's block a rank-B outer product dada_l^T . temb):
          "materialize"  the backward writes it into the flat gradient buffer like every other gradient (the only form in which the
                         gradient buffer is complete: accumulation, the autograd path and shard mode always use it);
          "factors"      it stays in factor form.  One GPU: the global norm takes its sum of squares from B x B Gram matrices and Adam
                         expands the product on the fly -- no 201 MB write, no two 201 MB reads per step; the adaLN weight blocks of
                         `gflat` are then NOT written.  Several GPUs (all-reduce mode): every rank all-gathers the factors
                         (B * (L * 4 D + Th) floats per rank, < 1 MB) instead of all-reducing the product (half of the wire), then
                         expands the summed gradient locally into `gflat`.
          "auto"         "factors" wherever it applies (adaptive norms, depth <= 32, all-reduce mode), unless VBX_ADALN_FACTORS=0.
        grad_mode: "allreduce" (DDP's exchange: every rank holds the summed gradient and runs the whole optimizer) or "shard"
        (reduce-scatter the buckets, each rank clips / Adams its 1 / world of the flat buffers, all-gather the updated fp32
        parameters, repack the operand copies in one pass): same results up to the summation order of the gradient norm, the
        optimizer's 3.3 GB of HBM traffic per step divided by the world size.

        Frozen parameters and LoRA adapters (one GPU).  The trainable set is the VoiceBox parameters with requires_grad=True, read
        here and re-derived whenever the tuple of flags differs from the cached one (a host comparison).  A frozen tensor keeps its
        bits, its m and v stay zero, it takes no part in the clip norm and gets no weight decay: the fused Adam runs over a filtered
        segment table and the norm over the trainable ranges only.  adaLN weights: all trainable -> the factor path as it is; all
        frozen -> no factor Adam, no Gram terms; mixed -> the step falls back to "materialize".  With adapters attached
        (VoiceBox.add_lora) the step runs vbx_lora_grad after the backward, takes the norm over the trainable ranges plus the adapter
        gradients, runs Adam on the adapters with the same coefficient and re-applies them (vbx_lora_apply).  With nothing frozen
        and no adapters every launch and table is what it was.  Anything frozen or adapted together with a gradient exchange
        (world > 1, VBX_FORCE_DIST) or grad_mode="shard" raises NotImplementedError, here or at the step that finds it.

        ema_decay (None: off -- nothing is allocated, every launch and table is what it was): an exponential moving average of the
        weights, kept in `self.ema` (fp32, the layout of the flat parameter buffer: `fp.offsets` index it) and updated INSIDE the Adam
        launches of every optimizer step, e' = fmaf(d, e - p', p') with d = ema_decay_at(self.steps) (include/vbx.h "EMA"): the fused
        pass, its filtered table, the factor-form launch, the plain launch of VBX_FUSED_ADAM=0 and the adapter Adam (on a second small
        buffer beside the adapters) all take their _ema entry point.  ema_update_after_step / ema_inv_gamma / ema_power: the decay
        schedule (dp.ema_decay_at; ema-pytorch's keywords, parity with that library unpinned).  The average starts as a copy of the
        weights (after the DP broadcast); ema_reset() copies them again.  A frozen tensor's average is not touched; with adapters the
        adapted matrices' slots of `self.ema` are frozen by construction and never read (the averaged W_eff is W0 + s . B_ema . A_ema).
        ema_state_dict() / load_ema_state_dict() / `with step.ema_weights():` see there.  grad_mode="shard" with ema_decay raises
        NotImplementedError: the owned chunks would need a gather before every use."""
        assert grad_mode in ("allreduce", "shard"), grad_mode
        assert adaln_grads in ("auto", "factors", "materialize"), adaln_grads
        check_ema_hyper(ema_decay, ema_update_after_step, ema_inv_gamma, ema_power)
        if ema_decay is not None and grad_mode == "shard":
            raise NotImplementedError("TrainStep: ema_decay is not served by grad_mode='shard' (each rank updates only the chunks it owns: the "
                                      "average would need an all-gather before every use) -- use grad_mode='allreduce'")
        self.ema_hyper = None if ema_decay is None else dict(ema_decay=float(ema_decay), ema_update_after_step=int(ema_update_after_step),
                                                             ema_inv_gamma=float(ema_inv_gamma),
                                                             ema_power=None if ema_power is None else float(ema_power))
        self.ema = None
        self._ema_swapped = False  # inside `with ema_weights():`
        self.grad_mode = grad_mode
        self.adaln_grads = adaln_grads
        self.wrapper, self.vb = wrapper, wrapper.voicebox
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        # wd > 0: AdamW as get_optimizer builds it (optimizer.py:10-35): decoupled decay p *= 1 - lr * wd on the parameters with
        # ndim >= 2 only (separate_weight_decayable_params), applied as one multi-tensor multiply in front of the fused Adam pass
        self.wd = float(wd)
        self._wd_params = [p for p in wrapper.voicebox.parameters() if p.requires_grad and p.ndim >= 2] if self.wd > 0 else []
        self.lr_schedule = lr_schedule  # e.g. WarmupCosineLR; an explicit `lr=` passed to step() wins
        self.grad_comm_dtype = grad_comm_dtype  # None / torch.float32: exact fp32 exchange (the reference's DDP); torch.bfloat16 halves it
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.fp = self.vb.flat_params()
        flat = self.fp.flat
        dev = flat.device
        if self.distributed and self.world > 1 and broadcast_params:
            dist.broadcast(flat, src=0, group=group)  # DDP's initial parameter broadcast (trainer.py:159)
            self._dirty()
        self.gflat = torch.zeros_like(flat)
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        if self.ema_hyper is not None:
            self.ema = torch.zeros_like(flat)
            self.ema.copy_(flat)
        self.sumsq = torch.zeros(1, device=dev)
        self.coef = torch.zeros(2, device=dev)
        self.scratch = torch.zeros(1024 + 32 * 64 * 64, device=dev)  # 1024 block partials + the L * B * B factor terms of the gradient norm
        self.steps = 0
        self.exchange = self.world > 1 or (force_dist() and self.distributed)
        self.comm_stream = torch.cuda.Stream(device=dev) if (self.exchange and dev.type == "cuda") else None
        self.bucket_bytes = bucket_bytes
        # length_bucket > 0: batches are padded (with masked frames) up to the next multiple of it, so that a dataset of varying
        # lengths (pad_to_longest collation, data.py:60-75) runs on a handful of engines instead of building a 3.6 GB activation
        # arena per distinct length.  Masked frames change nothing for the valid ones (the conv positional embedding, the attention
        # keys and the loss are all masked: voicebox_pytorch.py:220-233, attend.py:118-125, :1099-1115); 0 = exact lengths.
        self.length_bucket = int(length_bucket)
        self._stage_buf = None  # wire-dtype staging of the gradient exchange, allocated once (grad_comm_dtype only)
        self._flags = None   # (requires_grad per slot of fp.order, id of the attached LoRA state) the filter below was built from
        self._filter = None  # None: everything trainable, no adapters -- the step as it always was
        self._refresh_trainable()

    # -- frozen parameters and LoRA adapters
    def _refresh_trainable(self):
        """Re-derives the trainable set when the requires_grad flags (or the attached adapters) changed: host comparison, no sync."""
        fp = self.fp
        st = getattr(self.vb, "_lora", None)
        flags = (tuple(bool(fp.slots[s].requires_grad) for s in fp.order), id(st) if st is not None else None)
        if flags == self._flags:
            return
        on = flags[0]
        if all(on) and st is None:
            self._flags, self._filter, self._lora_rt = flags, None, None
            self._wd_params = [p for p in self.vb.parameters() if p.requires_grad and p.ndim >= 2] if self.wd > 0 else []
            return
        what = "LoRA adapters" if st is not None else "frozen parameters (requires_grad=False)"
        if self.exchange:
            raise NotImplementedError(f"TrainStep: {what} together with a gradient exchange (world size > 1 or VBX_FORCE_DIST) are not "
                                      "served: multi-rank fine-tuning is a follow-up -- fine-tune on one GPU")
        if self.grad_mode == "shard":
            raise NotImplementedError(f"TrainStep: {what} are not served by grad_mode='shard' -- use grad_mode='allreduce' on one GPU")
        by_slot = dict(zip(fp.order, on))
        rule = adaln_rule(by_slot, fp.depth)
        adaln_blocks = self.adaln_weight_ranges() if any(s.endswith(".G1W") for s in fp.order) else []
        ranges = trainable_ranges(fp, on)
        ranges_fa = trainable_ranges(fp, on, exclude=adaln_blocks)  # what is read from gflat when the adaLN blocks are in factor form
        if rule == "all" and not ranges_fa and st is None:
            rule = "mixed"  # nothing but adaLN weights is trainable: the norm launch needs a range, so take the materialised gradient
        # (with the padding up to the next slot, so that what is left of a plain segment starts on a slot boundary: 16-byte accesses)
        frozen = [(fp.offsets[s], (fp.offsets[s] + fp.slots[s].numel() + 63) // 64 * 64) for s, f in zip(fp.order, on) if not f]
        self._filter = dict(key=flags, ranges=ranges, ranges_factor=ranges_fa, adaln=rule, frozen=frozen, any_base=any(on))
        self._wd_params = [p for p in self.vb.parameters() if p.requires_grad and p.ndim >= 2] if self.wd > 0 else []
        self._lora_rt = None
        if st is not None:
            dev = fp.flat.device
            lflat = st.ensure(dev)
            tab = st.table()
            old = getattr(self, "_lora_keep", None)  # the moments survive a refresh that keeps the same adapters
            if old is not None and old["state"] is st and old["m"].numel() == lflat.numel() and old["m"].device == dev:
                self._lora_rt = old
            else:
                self._lora_rt = dict(state=st, g=torch.zeros_like(lflat), m=torch.zeros_like(lflat), v=torch.zeros_like(lflat),
                                     scratch=torch.zeros(max(1, tab.scratch_floats), device=dev))
                if self.ema is not None:  # the adapters' average: lflat's layout, starts as a copy, kept like m / v
                    self._lora_rt["ema"] = lflat.detach().clone()
            self._lora_keep = self._lora_rt
        self._flags = flags

    def _dirty(self, keep=None):
        """The flat parameter buffer was written behind PyTorch's version counters (native Adam, broadcast): bump the weights
        epoch, which EVERY engine compares in bind_params -- including engines evicted from `vb._engines` that a cached
        MidpointSampler still holds.  `keep` had its packed copies refreshed in the same pass."""
        self.fp.bump()
        if keep is not None:
            keep.packed_version = self.fp.weights_key()

    # -- EMA of the weights (ema_decay=): kept by the Adam launches themselves, see __init__
    def ema_decay_at(self, t):
        """The decay of optimizer step t (1-based) under this step's schedule: dp.ema_decay_at with the constructor's keywords."""
        self._require_ema("ema_decay_at")
        return ema_decay_at(t, **self.ema_hyper)

    def _require_ema(self, what):
        if self.ema is None:
            raise RuntimeError(f"TrainStep.{what}: this step keeps no average (build it with ema_decay=)")

    def _refuse_inside_ema_weights(self, what):
        if self._ema_swapped:
            raise RuntimeError(f"TrainStep.{what} inside `with ema_weights():` -- the flat buffer holds the average there, not the "
                               "optimizer's iterate; leave the context first")

    def _ema_launch_args(self):
        """What engine.adam_step_packed takes beside its arguments when the average is on (nothing otherwise)."""
        if self.ema is None:
            return {}
        return dict(ema=self.ema, ema_decay=self.ema_decay_at(self.steps))

    def _lora_ema(self):
        """(lflat, its average) with adapters attached, else None."""
        self._refresh_trainable()
        lo = self._lora_rt
        if lo is None or self.ema is None:
            return None
        return lo["state"].ensure(self.fp.flat.device), lo["ema"]

    def ema_reset(self):
        """The average becomes a copy of the weights again: after weights were written behind the step (load_state_dict, a
        broadcast), which the average cannot know about."""
        self._require_ema("ema_reset")
        self._refuse_inside_ema_weights("ema_reset")
        self.ema.copy_(self.fp.flat)
        la = self._lora_ema()
        if la is not None:
            la[1].copy_(la[0])

    def _ema_views(self):
        """{state-dict key: view of the average with the parameter's shape} for every flat-backed parameter and every adapter."""
        fp = self.fp
        by_id = {id(fp.slots[s]): s for s in fp.order}
        la = self._lora_ema()
        adapters = {}
        if la is not None:
            for e in self._lora_rt["state"].entries:
                adapters[id(e["module"].lora_A)], adapters[id(e["module"].lora_B)] = e["a_off"], e["b_off"]
        out = {}
        for k, p in self.vb.named_parameters(remove_duplicate=False):
            if id(p) in by_id:
                o = fp.offsets[by_id[id(p)]]
                out[k] = self.ema[o:o + p.numel()].view(p.shape)
            elif id(p) in adapters:
                o = adapters[id(p)]
                out[k] = la[1][o:o + p.numel()].view(p.shape)
        return out

    def ema_state_dict(self):
        """The averaged model, keyed like vb.state_dict(): clones out of the average for every flat-backed parameter, the live tensors
        for everything else (null_cond, buffers).  With adapters attached W0 sits under the reference's keys and the averaged
        lora_A / lora_B are included, exactly as state_dict() does for the live ones.  (Inside `with ema_weights():` the model's own
        state dict is that already: clones of it.)"""
        self._require_ema("ema_state_dict")
        sd = self.vb.state_dict()
        if self._ema_swapped:
            return type(sd)((k, v.detach().clone()) for k, v in sd.items())
        adapted = set()
        st = getattr(self.vb, "_lora", None)
        if st is not None:
            adapted = {e["key"] for e in st.entries}  # W0 stands there (the state-dict hook): not the slot of the average
        for k, view in self._ema_views().items():
            if k in sd and k not in adapted:
                sd[k] = view.detach().clone()
        return sd

    def load_ema_state_dict(self, sd):
        """The inverse of ema_state_dict(): every flat-backed parameter's (and adapter's) entry is copied into the average; the other
        keys are not the average's business.  A missing key or a shape mismatch raises ValueError before anything is copied."""
        self._require_ema("load_ema_state_dict")
        self._refuse_inside_ema_weights("load_ema_state_dict")
        st = getattr(self.vb, "_lora", None)
        adapted = {e["key"] for e in st.entries} if st is not None else set()
        views = {k: v for k, v in self._ema_views().items() if k not in adapted}
        missing = sorted(k for k in views if k not in sd)
        if missing:
            raise ValueError(f"load_ema_state_dict: missing keys {missing}")
        for k, view in views.items():
            if tuple(sd[k].shape) != tuple(view.shape):
                raise ValueError(f"load_ema_state_dict: {k} has shape {tuple(sd[k].shape)}, the parameter has {tuple(view.shape)}")
        with torch.no_grad():
            for k, view in views.items():
                view.copy_(sd[k])

    def _ema_swap(self, entering):
        """flat <-> ema (and the adapters <-> their average) in place, vbx_swap_f32: the addresses stay, so engines and captured graphs
        stay valid and only repack (fp.bump)."""
        st = _lib.current_stream()
        flat = self.fp.flat
        la = self._lora_ema()
        _lib.call("vbx_swap_f32", flat, self.ema, flat.numel(), st)
        if la is not None:
            _lib.call("vbx_swap_f32", la[0], la[1], la[0].numel(), st)
            if entering:
                # the adapted slots hold what the average's (never updated) slots held: W_eff = W0 + s . B_ema . A_ema into them.
                # On the way out the swap itself brings the live W_eff back bit for bit.
                state = self._lora_rt["state"]
                state.needs_apply = True
                state.apply()
        self.fp.bump()

    def ema_weights(self):
        """`with step.ema_weights():` -- the averaged model is served by every path that reads the weights (wrapper(...) in eval,
        wrapper.sample(...), cached and captured samplers, state_dict()): the flat buffer and the average change places in place.  On
        exit (also after an exception) they change back: the weights are bit-equal to before.  Nesting, and step() / accumulate*()
        inside, raise RuntimeError."""
        import contextlib

        self._require_ema("ema_weights")

        @contextlib.contextmanager
        def ctx():
            if self._ema_swapped:
                raise RuntimeError("TrainStep.ema_weights: already inside `with ema_weights():` (the context does not nest)")
            self._ema_swap(True)
            self._ema_swapped = True
            try:
                yield self
            finally:
                self._ema_swapped = False
                self._ema_swap(False)

        return ctx()

    # -- gradient accumulation with a deferred exchange (VoiceBoxTrainer.train_step, trainer.py:258-272: every micro-batch but
    #    the last runs under accelerator.no_sync, the loss is divided by grad_accum_every)
    def accumulate(self, x1, weight, mask=None, cond_token_ids=None, input_sampling_rate=None, lens=None, wave_lens=None, token_lens=None):
        """forward + backward of one micro-batch; gradients * weight are added to the accumulation buffer (no exchange).
        lens: see step."""
        self._refuse_inside_ema_weights("accumulate")
        self._refresh_trainable()
        if getattr(self, "gacc", None) is None:
            self.gacc = torch.zeros_like(self.gflat)
            self.acc_coef = torch.zeros(1, device=self.gflat.device)
            self.acc_pending = False
        loss = self._forward_backward(x1, mask, cond_token_ids, on_stage=None, input_sampling_rate=input_sampling_rate, lens=lens,
                                      wave_lens=wave_lens, token_lens=token_lens)
        self.acc_coef.fill_(float(weight))
        n = self.gflat.numel()
        _lib.call("vbx_axpy_dev", self.gacc, self.gflat, self.acc_coef, 0, self.gacc, n, _lib.current_stream())
        self.acc_pending = True
        return loss

    FACTOR_MAX_BATCH = 64  # vbx_sumsq_adaln_factors (one GPU: B x B Gram terms per layer) serves local batches up to this size

    def adaln_factors_apply(self, batch=None):
        """True when step() keeps the adaLN weight gradients in factor form (see __init__).  `batch`: the local batch size of the
        step being decided; on ONE GPU the factor-form gradient norm is a B x B Gram sum whose kernel serves B <= 64, so a larger
        batch falls back to the materialised gradient in "auto" mode (it used to raise after the backward)."""
        if self.adaln_grads == "materialize" or self.grad_mode == "shard":
            return False
        if self._filter is not None and self._filter["adaln"] == "mixed":
            return False  # some adaLN weights frozen, some not: the factor kernels serve whole blocks, so the gradient is materialised
        if self.adaln_grads == "auto" and os.environ.get("VBX_ADALN_FACTORS", "1") == "0":
            return False
        c = self.vb._cfg
        ok = not c.get("plain_norm") and not c.get("stack_only") and c["L"] <= 32 and self.fp.flat.is_cuda
        if batch is not None and not self.exchange and batch > self.FACTOR_MAX_BATCH:
            ok = False
        assert ok or self.adaln_grads == "auto", ("adaln_grads='factors' needs a VoiceBox with adaptive norms (depth <= 32) on a GPU"
                                                  " and, on one GPU, a batch of at most 64")
        return bool(ok)

    def adaln_weight_ranges(self):
        """Flat ranges [lo, hi) of every layer's adaLN projection weight block (G1W | B1W | G2W | B2W, contiguous)."""
        fp = self.fp
        out = []
        for l in range(fp.depth):
            lo = fp.offsets[f"L{l}.G1W"]
            hi = fp.offsets[f"L{l}.B2W"] + fp.slots[f"L{l}.B2W"].numel()
            out.append((lo, hi))
        return sorted(out)

    def _reducer(self, comm_dtype=None, skip_adaln=False):
        red = GradBucketReducer(self.gflat, self.fp.stage_ranges, group=self.group, bucket_bytes=self.bucket_bytes,
                                comm_stream=self.comm_stream, comm_dtype=comm_dtype, stage_buf=self._stage_buf,
                                shard=self.grad_mode == "shard" and self.exchange,
                                skip_ranges=self.adaln_weight_ranges() if skip_adaln else ())
        self._red = red
        return red

    def _exchange_adaln_factors(self, eng):
        """Data-parallel exchange of the adaLN weight gradients in factor form: all-gather every rank's dada [L, B, 4 D] and temb
        [B, Th] (one small collective), then expand the SUM over ranks, sum_r dada_r^T . temb_r = dada_all^T . temb_all, into the
        adaLN weight blocks of the flat gradient buffer on every rank -- what the all-reduce of the products would have left there."""
        from .engine import _rt, _check
        _, _, woff, _, J4, Th = eng.adaln_factor_info()
        dada, temb = eng.adaln_factor_tensors()  # views of the engine's activation arena
        dada_all, temb_all, self.factor_wire_floats = gather_adaln_factors(dada, temb, self.group)  # (world 1 + VBX_FORCE_DIST: no-op gather)
        st = _lib.current_stream()
        for l in range(eng.cfg["L"]):
            _check(_rt().vbx_adaln_expand_dw(temb_all.data_ptr(), dada_all[l].data_ptr(), self.gflat.data_ptr() + 4 * int(woff[l]),
                                             dada_all.shape[1], Th, J4, 0, st), "vbx_adaln_expand_dw")
        self._keep_factors = (dada_all, temb_all)  # alive until the launches have run

    def accumulate_last_and_apply(self, x1, weight, mask=None, cond_token_ids=None, lr=None, input_sampling_rate=None, lens=None,
                                  wave_lens=None, token_lens=None):
        """The LAST micro-batch of an accumulation window, with the exchange overlapped with its backward (DDP leaves `no_sync`
        for exactly this micro-batch, trainer.py:258-272): as each backward stage completes, its slice of the accumulator is
        folded in (g = acc + weight * g) and the bucketed all-reduce of that slice starts while earlier layers are still running --
        instead of exchanging all 410 MB after the backward with nothing to overlap (apply_accumulated).  Then clip + Adam."""
        self._refuse_inside_ema_weights("accumulate_last_and_apply")
        self._refresh_trainable()
        if getattr(self, "gacc", None) is None or not getattr(self, "acc_pending", False):
            self.gacc = torch.zeros_like(self.gflat) if getattr(self, "gacc", None) is None else self.gacc
        red = self._reducer(self.grad_comm_dtype)

        def on_stage(i, rng=None):
            lo, hi = rng if rng is not None else self.fp.stage_ranges[i]
            g, a = self.gflat[lo:hi], self.gacc[lo:hi]
            torch.add(a, g, alpha=float(weight), out=g)  # g = acc + weight * g, in place on the stage's slice
            if self.exchange:
                red.stage_done(i, rng)

        loss = self._forward_backward(x1, mask, cond_token_ids, on_stage=on_stage, input_sampling_rate=input_sampling_rate, lens=lens,
                                      wave_lens=wave_lens, token_lens=token_lens)
        red.finish()
        self._stage_buf = red.stage_buf
        self.gacc.zero_()
        self.acc_pending = False
        self._clip_adam(self._last_eng, lr)
        return loss

    def apply_accumulated(self, lr=None):
        """all-reduce (sum) of the accumulated gradients, clip, Adam; clears the accumulator.  (No backward is left to overlap the
        exchange with: prefer accumulate_last_and_apply for the window's last micro-batch.)"""
        self._refuse_inside_ema_weights("apply_accumulated")
        assert getattr(self, "acc_pending", False), "nothing accumulated"
        self._refresh_trainable()
        self.gflat.copy_(self.gacc)
        self.gacc.zero_()
        self.acc_pending = False
        if self.exchange:
            red = self._reducer(self.grad_comm_dtype)
            for i, rng in enumerate(self.fp.stage_ranges):
                red.stage_done(i, rng)
            red.finish()
            self._stage_buf = red.stage_buf
        self._clip_adam(self._last_eng, lr)

    def _forward_backward(self, x1, mask, cond_token_ids, on_stage, adaln_factors=False, sq_fold=False, input_sampling_rate=None,
                          lens=None, wave_lens=None, token_lens=None):
        from . import wave_lens as wl
        from .engine import precise_enabled

        vb, w = self.vb, self.wrapper
        dev = self.fp.flat.device
        st = _lib.current_stream
        key_lens = None
        # per-row token counts (wave_lens.py): every refusal, and the host check of the values, before anything is launched
        wl.refuse_token_lens(token_lens, lens is not None or wave_lens is not None, cond_token_ids if vb.condition_on_text else None,
                             None, "TrainStep")
        if token_lens is not None:
            if precise_enabled():
                raise NotImplementedError("TrainStep: token_lens is not served in precise mode")
            token_lens = wl.token_lens_device(token_lens, cond_token_ids.shape[0], cond_token_ids.shape[-1], dev, "TrainStep")
        if wave_lens is not None:  # a ragged batch of WAVES (wave_lens.py): refusals first, rows encoded as the row alone, then lens=
            w2v = getattr(w, "wav2vec", None)
            from_w2v = cond_token_ids is None and vb.condition_on_text and w2v is not None
            wl.refuse(wave_lens, x1, None, lens, mask, vb.audio_enc_dec, "TrainStep",
                      wav2vec_ids=from_w2v and wl.wav2vec_lacks(w2v) is not None, wav2vec=w2v)
            if from_w2v:  # the ids of every row alone and their counts (HubertWithKmeans(lens=)), from the waves as they were given
                if precise_enabled():
                    raise NotImplementedError("TrainStep: wave_lens with token ids from wav2vec= resizes each row's ids to its own "
                                              "frames, which precise mode does not serve")
                cond_token_ids, token_lens = w.wav2vec_token_ids(x1, input_sampling_rate, wave_lens=wave_lens)
                token_lens = wl.token_lens_device(token_lens, cond_token_ids.shape[0], cond_token_ids.shape[-1], dev, "TrainStep")
            x1, _, lens = w.encode_raw_audio(x1, None, input_sampling_rate, wave_lens=wave_lens)
        if lens is not None:  # a ragged batch by lengths (train_lens.py): refusals and host validation before anything is launched
            from . import train_lens

            train_lens.refuse_with_mask(lens, mask, "TrainStep")
            train_lens.refuse_raw_audio(lens, x1, "TrainStep")
            lens = train_lens.frame_lens(lens, x1.shape[0], x1.shape[1], dev)
            mask = train_lens.prefix_mask(lens, x1.shape[1])
            # the frames added up to length_bucket below lie past every length: key_lens is unchanged by that padding
            key_lens = train_lens.key_lens(lens, vb._cfg["R"])
        # a wave batch of a codec model (voicebox_pytorch.py:1349-1371), resampled first when the wrapper says so; latents pass through
        if cond_token_ids is None and vb.condition_on_text and getattr(w, "wav2vec", None) is not None and x1.ndim in (2, 3) \
                and (x1.ndim == 2 or x1.shape[1] == 1):
            cond_token_ids = w.wav2vec_token_ids(x1, input_sampling_rate)  # :1386-1388: semantic ids of the wave itself
        x1, _ = w.encode_raw_audio(x1, None, input_sampling_rate)
        x1 = x1.to(dev, torch.float32).contiguous()
        B, N, _ = x1.shape
        if mask is not None:
            mask = mask.to(dev)  # a DataLoader hands over CPU masks; the kernels take device pointers only
        # --- ConditionalFlowMatcherWrapper.forward, same RNG draw order (voicebox_pytorch.py:1399,1403,1025,146)
        x0 = take_draw("x0")
        x0 = torch.randn_like(x1) if x0 is None else x0.to(dev, torch.float32)
        times = take_draw("times")
        times = torch.rand((B,), dtype=torch.float32, device=dev) if times is None else times.to(dev, torch.float32)
        vb.train()
        frac = take_draw("frac_lengths")
        if frac is None:
            frac = torch.empty((B,), dtype=torch.float32, device=dev).uniform_(*vb.frac_lengths_mask)
        # a bool [B, N] padding mask joins the launch; any other (token resolution, another dtype) takes the torch expression below
        pad_in = mask is not None and mask.dtype == torch.bool and tuple(mask.shape) == (B, N)
        wt, flow, cond_mask, loss_mask = self._cfm_inputs_and_masks(x1, x0, times, frac.to(dev), mask if pad_in else None, key_lens)
        text = None
        if vb.condition_on_text:  # cond_drop_prob draw comes after the span-mask draws (voicebox_pytorch.py:1025,1040-1041)
            from .masks import prob_mask_like

            assert cond_token_ids is not None, "a text-conditioned model trains on cond_token_ids"
            drop = None
            if w.cond_drop_prob > 0.:
                drop = take_draw("cond_drop")
                drop = prob_mask_like((B,), w.cond_drop_prob, dev) if drop is None else drop.to(dev)
            ids = cond_token_ids.to(dev)
            if mask is not None and ids.shape[-1] != N and mask.shape[-1] != N:
                # voicebox_pytorch.py:1064-1066: the key-padding mask follows the token ids to frame resolution
                m4 = mask.float()[:, None, :, None]
                mask = torch.nn.functional.interpolate(m4, (N, 1), mode="bilinear")[:, 0, :, 0].to(torch.bool)
            text = (ids, vb.null_cond_id, drop, vb.null_cond, token_lens)
        if mask is not None and not pad_in:
            loss_mask = cond_mask & mask  # reduce_masks_with_and (:1099)
        if self.length_bucket > 0 and N % self.length_bucket and text is None:  # (token ids are resized to the frame count: :1055-1062)
            Nb = -(-N // self.length_bucket) * self.length_bucket
            pad = Nb - N
            padf = lambda t: torch.nn.functional.pad(t, (0, 0, 0, pad))           # (B, N, D) -> (B, Nb, D), zeros
            padm = lambda t: torch.nn.functional.pad(t, (0, pad), value=False)    # (B, N) -> (B, Nb), False
            wt, flow = padf(wt), padf(flow)
            mask = padm(mask if mask is not None else torch.ones(B, N, dtype=torch.bool, device=dev))
            cond_mask, loss_mask = padm(cond_mask), padm(loss_mask)
            N = Nb
        eng = vb.engine(B, N, training=True)
        loss = eng.forward(wt, flow, cond_mask, times, attn_mask=mask, target=flow, loss_mask=loss_mask, text=text, key_lens=key_lens)
        sq = None
        if sq_fold and adaln_factors and on_stage is None and eng.sq_partials_info()[0] > 0:
            need = eng.sumsq_scratch_floats(True)
            if self.scratch.numel() < need:
                self.scratch = torch.zeros(need, device=dev)
            sq = eng.sq_partials_ptr(self.scratch)
        self._sq_folded = sq is not None  # the norm of THIS backward's big weight matrices is already in self.scratch
        eng.backward(self.gflat, gscale=None, on_stage=on_stage, adaln_factors=adaln_factors, sq_partials=sq)
        self._last_eng = eng
        return loss

    def _cfm_inputs_and_masks(self, x1, x0, times, frac, mask, key_lens):
        """(w, flow, cond_mask, loss_mask) of the CFM objective from the drawn numbers: w and flow (:1404-1410), the span mask
        mask_from_frac_lengths(N, frac) with its `rand` draw (:146) and loss_mask = cond_mask & mask (reduce_masks_with_and, :1099) in ONE
        launch, vbx_cfm_inputs_masks -- byte for byte what masks.py computes with a dozen torch launches."""
        w, dev = self.wrapper, x1.device
        B, N, _ = x1.shape
        wt, flow = torch.empty_like(x1), torch.empty_like(x1)
        rand = take_draw("rand")  # the draw of mask_from_frac_lengths, at the same place in the order of draws
        rand = torch.empty((B,), dtype=torch.float32, device=dev).uniform_(0, 1) if rand is None else rand.to(dev).float()
        frac = frac.float().contiguous()
        pad = None
        if mask is not None:
            assert mask.dtype == torch.bool and tuple(mask.shape) == (B, N), (mask.dtype, tuple(mask.shape), (B, N))
            pad = mask.contiguous()
        cond_mask = torch.empty((B, N), dtype=torch.bool, device=dev)
        loss_mask = cond_mask if pad is None else torch.empty((B, N), dtype=torch.bool, device=dev)
        _lib.call("vbx_cfm_inputs_masks", x1, x0.contiguous(), times.contiguous(), float(w.sigma), wt, flow, B, x1[0].numel(), frac,
                  rand.contiguous(), pad, key_lens if pad is not None else None, self.vb._cfg["R"], N, cond_mask,
                  loss_mask if pad is not None else None, _lib.current_stream())
        return wt, flow, cond_mask, loss_mask

    def _clip_adam_sharded(self, eng, lr, red):
        """grad_mode="shard": this rank holds the summed gradient of its chunks only (red.owned).  Global norm = sum over ranks of
        the chunk sums of squares (all-gathered and added in rank order: every rank computes the same coefficient), Adam on the
        owned chunks of (p, m, v), all-gather of the updated parameters, one repack of the operand copies."""
        st = _lib.current_stream
        dev = self.gflat.device
        part = torch.zeros(len(red.owned) + 1, device=dev)
        for i, (lo, hi) in enumerate(red.owned):
            _lib.call("vbx_sumsq", self.gflat[lo:hi], hi - lo, part[i:i + 1], self.scratch, st())
        mine = part[:len(red.owned)].sum().reshape(1)
        parts = [torch.zeros(1, device=dev) for _ in range(self.world)]
        dist.all_gather(parts, mine, group=self.group)  # W scalars; the list form exists on every backend
        self.sumsq.copy_(torch.cat(parts).sum().reshape(1))  # added in rank order: the same coefficient on every rank
        _lib.call("vbx_clip_coef", self.sumsq, float(self.max_grad_norm or 0.0), 1.0 / self.world, self.coef, st())
        rate = float(lr if lr is not None else self.lr)
        if self._wd_params:
            with torch.no_grad():
                torch._foreach_mul_(self._wd_params, 1.0 - rate * self.wd)  # replicated (elementwise, identical on every rank)
        flat = self.fp.flat
        for lo, hi in red.owned:
            _lib.call("vbx_adam_step", flat[lo:hi], self.gflat[lo:hi], self.m[lo:hi], self.v[lo:hi], hi - lo, rate,
                      float(self.betas[0]), float(self.betas[1]), float(self.eps), self.steps, self.coef, st())
        red.all_gather(flat)
        self._dirty()  # every engine (this one included) repacks its fp16 / bf16 operand copies on its next bind_params

    def gather_optimizer_state(self):
        """grad_mode="shard": the Adam moments of a chunk live on its owner only; before a checkpoint every rank collects all of them
        (no-op in all-reduce mode)."""
        red = getattr(self, "_red", None)
        if self.grad_mode == "shard" and red is not None:
            red.all_gather(self.m)
            red.all_gather(self.v)

    def _clip_adam(self, eng, lr, adaln_factors=False):
        # --- clip (global norm of the rank-averaged gradient) + Adam, all on device, no host sync
        # adaln_factors (one GPU): the adaLN weight blocks of gflat were not written; their share of the norm and their Adam update
        # come from the factors left in `eng`'s arena (include/vbx.h "FACTOR form")
        st = _lib.current_stream
        n = self.gflat.numel()
        if lr is None and self.lr_schedule is not None:
            lr = self.lr_schedule.rate_for_step(self.steps)
        self.steps += 1
        red = getattr(self, "_red", None)
        if self.grad_mode == "shard" and red is not None and red.shard and red.active:
            return self._clip_adam_sharded(eng, lr, red)
        if self._filter is not None:
            return self._clip_adam_filtered(eng, lr, adaln_factors)
        if adaln_factors:
            folded = getattr(self, "_sq_folded", False)
            if not folded and self.scratch.numel() < eng.sumsq_scratch_floats(False):  # (folded: sized before the backward wrote into it)
                self.scratch = torch.zeros(eng.sumsq_scratch_floats(False), device=self.scratch.device)
            eng.sumsq_with_adaln_factors(self.gflat, self.sumsq, self.scratch, sq_fold=folded)
        else:
            _lib.call("vbx_sumsq", self.gflat, n, self.sumsq, self.scratch, st())
        _lib.call("vbx_clip_coef", self.sumsq, float(self.max_grad_norm or 0.0), 1.0 / self.world, self.coef, st())
        if self._wd_params:
            with torch.no_grad():
                torch._foreach_mul_(self._wd_params, 1.0 - float(lr if lr is not None else self.lr) * self.wd)
            # the in-place multiply bumped the parameters' version counters; the fused pass below rewrites every operand copy from
            # the updated values anyway, so the training engine need not repack first
            eng.packed_version = self.fp.weights_key()
        # Adam + refresh of the training engine's fp16/bf16 operand copies in one pass (other engines repack lazily)
        if os.environ.get("VBX_FUSED_ADAM", "1") != "0":
            eng.adam_step_packed(self.gflat, self.m, self.v, float(lr if lr is not None else self.lr), self.betas[0], self.betas[1],
                                 self.eps, self.steps, self.coef, adaln_factors=adaln_factors,
                                 **self._ema_launch_args())  # bumps the weights epoch; `eng` stays current
        else:  # A/B: plain Adam, the next forward repacks every weight
            assert not adaln_factors, "VBX_FUSED_ADAM=0 needs the materialised gradient: set VBX_ADALN_FACTORS=0 too"
            self._dirty()
            hyper = (n, float(lr if lr is not None else self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), self.steps,
                     self.coef, st())
            if self.ema is None:
                _lib.call("vbx_adam_step", self.fp.flat, self.gflat, self.m, self.v, *hyper)
            else:
                _lib.call("vbx_adam_step_ema", self.fp.flat, self.gflat, self.m, self.v, self.ema, self.ema_decay_at(self.steps), *hyper)

    def _sumsq_filtered(self, eng, factor_terms):
        """self.sumsq[0] = sum of squares over the trainable ranges of gflat (+ the adaLN Gram terms when those blocks are trainable and
        in factor form, + the adapter gradient buffer): vbx_sumsq_ranges in launches of at most 64 ranges, every launch but the last
        leaving its sum behind the Gram terms in the scratch, where the last one picks them up as extra values."""
        import ctypes as C
        from .engine import _rt, _check
        f, lo = self._filter, self._lora_rt
        st = _lib.current_stream()
        nterms = eng.cfg["L"] * eng.B * eng.B if factor_terms else 0
        launches = [(self.gflat, ch) for ch in range_chunks(f["ranges_factor"] if factor_terms else f["ranges"])]
        if lo is not None:
            launches.append((lo["g"], [(0, lo["g"].numel())]))
        assert launches, "nothing is trainable"
        need = 1024 + nterms + len(launches)
        if self.scratch.numel() < need:
            self.scratch = torch.zeros(need, device=self.scratch.device)
        if factor_terms:
            dada, temb, _, _, J4, Th = eng.adaln_factor_info()
            _check(_rt().vbx_sumsq_adaln_factors(dada, temb, eng.cfg["L"], eng.B, J4, Th, self.scratch.data_ptr() + 4 * 1024, st),
                   "vbx_sumsq_adaln_factors")
        for i, (buf, ch) in enumerate(launches):
            last = i + 1 == len(launches)
            arr = (C.c_long * (2 * len(ch)))(*[x for r in ch for x in r])
            out = self.sumsq.data_ptr() if last else self.scratch.data_ptr() + 4 * (1024 + nterms + i)
            _check(_rt().vbx_sumsq_ranges(buf.data_ptr(), arr, len(ch), (nterms + i) if last else 0, out, self.scratch.data_ptr(), st),
                   "vbx_sumsq_ranges")

    def _clip_adam_filtered(self, eng, lr, adaln_factors):
        """clip + Adam of a partly frozen and / or adapted model (one GPU): vbx_lora_grad, the norm over what is trainable,
        vbx_clip_coef, the filtered fused Adam on the base, vbx_adam_step on the adapters with the same coefficient, vbx_lora_apply."""
        f, lo = self._filter, self._lora_rt
        st = _lib.current_stream
        rate = float(lr if lr is not None else self.lr)
        factor_terms = bool(adaln_factors) and f["adaln"] == "all"
        if lo is not None:
            state = lo["state"]
            lflat = state.ensure(self.fp.flat.device)
            state.table().grad(self.gflat, lflat, lo["g"], lo["scratch"])
        self._sumsq_filtered(eng, factor_terms)
        _lib.call("vbx_clip_coef", self.sumsq, float(self.max_grad_norm or 0.0), 1.0 / self.world, self.coef, st())
        if self._wd_params:
            with torch.no_grad():
                torch._foreach_mul_(self._wd_params, 1.0 - rate * self.wd)
            eng.packed_version = self.fp.weights_key()  # (as in _clip_adam; with adapters the apply below makes every engine repack)
        if f["any_base"]:
            eng.adam_step_packed(self.gflat, self.m, self.v, rate, self.betas[0], self.betas[1], self.eps, self.steps, self.coef,
                                 adaln_factors=adaln_factors, trainable=f, factor_adam=factor_terms, **self._ema_launch_args())
        if lo is not None:
            hyper = (lflat.numel(), rate, float(self.betas[0]), float(self.betas[1]), float(self.eps), self.steps, self.coef, st())
            if self.ema is None:
                _lib.call("vbx_adam_step", lflat, lo["g"], lo["m"], lo["v"], *hyper)
            else:
                _lib.call("vbx_adam_step_ema", lflat, lo["g"], lo["m"], lo["v"], lo["ema"], self.ema_decay_at(self.steps), *hyper)
            state.needs_apply = True
            state.apply()  # W_eff = W0 + s . B . A into the master slots; bumps the weights epoch: every engine and sampler repacks

    def step(self, x1, mask=None, lr=None, cond_token_ids=None, input_sampling_rate=None, lens=None, wave_lens=None, token_lens=None):
        """x1: (B_local, frames, dim) on this rank's GPU, or a wave batch (B_local, samples) for a model built with audio_enc_dec
        (cond_token_ids (B_local, tokens) for a text-conditioned model); input_sampling_rate: the rate of such waves, for a wrapper built
        with resample_input=True.
        lens: a list, a CPU int tensor or a device int tensor [B_local] of frame counts instead of mask -- the same step as
        mask = arange(frames) < lens[:, None], bit for bit, with the attention forward and backward stopping at each row's length
        (ConditionalFlowMatcherWrapper.forward).  With text conditioning it counts frames, not tokens.
        wave_lens: x1 is a padded batch of waves and row b holds wave_lens[b] real samples at the rate the waves are given in -- every
        row is encoded as the row alone and the step runs as step(latents, lens=codec.frame_lens(...)); not with lens or mask.  A
        text-conditioned model without cond_token_ids takes them, and token_lens, from a wav2vec= that serves lengths.
        token_lens: with lens or wave_lens and cond_token_ids, the token count of each row -- row b's first token_lens[b] ids are
        resized to row b's own frames (ConditionalFlowMatcherWrapper.forward).
        Returns the (un-synchronised) local loss tensor."""
        # --- backward with overlapped gradient exchange
        self._refuse_inside_ema_weights("step")
        self._refresh_trainable()
        factors = self.adaln_factors_apply(batch=int(x1.shape[0])) and os.environ.get("VBX_FUSED_ADAM", "1") != "0"
        red = self._reducer(self.grad_comm_dtype, skip_adaln=factors and self.exchange)
        # one GPU, factor form: the slab reduce also leaves the sums of squares of what it stores (no second pass over the big
        # weight gradients for the clip norm); VBX_SUMSQ_FOLD=0: A/B
        # (a partly frozen or adapted model takes the plain path: the fold's partials cover all four big matrices of every layer)
        fold = factors and not self.exchange and os.environ.get("VBX_SUMSQ_FOLD", "1") != "0" and self._filter is None
        loss = self._forward_backward(x1, mask, cond_token_ids, on_stage=red.stage_done if self.exchange else None, adaln_factors=factors,
                                      sq_fold=fold, input_sampling_rate=input_sampling_rate, lens=lens, wave_lens=wave_lens,
                                      token_lens=token_lens)
        if factors and self.exchange:  # the factors travel (one small all-gather) while the last buckets are still in flight
            self._exchange_adaln_factors(self._last_eng)
        red.finish()
        self._stage_buf = red.stage_buf
        self.wire_bytes = (red.wire_floats * (2 if self.grad_comm_dtype == torch.bfloat16 else 4)
                           + 4 * getattr(self, "factor_wire_floats", 0) * (1 if factors and self.exchange else 0)) if self.exchange else 0
        # one GPU: clip + Adam straight from the factors; several: the expanded sum is in gflat like any other gradient
        self._clip_adam(self._last_eng, lr, adaln_factors=factors and not self.exchange)
        return loss
