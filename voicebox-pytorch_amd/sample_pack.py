"""Host side of sample(lens=, pack=True) (model.ConditionalFlowMatcherWrapper.sample): the packed row layout of include/vbx.h
("packed rows"), its plan and the two index ops that move a padded batch into it and back.  Pure torch, runs on the CPU; nothing
here launches a forward -- the packed sampler is solver.PackedMidpointSampler / PackedRKSampler.

A ragged batch [B, N] with lengths len_b runs as ONE batch row of Mp rows.  Row b becomes a segment: R register rows, len_b frame
rows, then dead rows up to the next multiple of PACK_ALIGN = 128 (the attention query tile), segments in batch order; with
pack_bucket Mp is rounded up to a multiple of it and the rows past the last segment are dead."""
from collections import namedtuple

import torch

PACK_ALIGN = 128  # VBX_PACK_ALIGN: rows of an attention query tile, two conv_embed chunks

PackPlan = namedtuple("PackPlan", "Mp B N R lens seg_start seg_klen tile_seg src_row dst_row local_row live_rows dead_rows padded_rows")


def check_pack_bucket(pack_bucket):
    if pack_bucket is None:
        return None
    if isinstance(pack_bucket, bool) or not isinstance(pack_bucket, int) or pack_bucket < PACK_ALIGN or pack_bucket % PACK_ALIGN:
        raise ValueError(f"pack_bucket must be a positive multiple of {PACK_ALIGN} (the packed row count is rounded up to it), "
                         f"got {pack_bucket!r} -- pass a multiple of {PACK_ALIGN}, or None for the exact packed size")
    return pack_bucket


def packed_rows(lens, R, pack_bucket=None):
    """Mp of a batch with these lengths: sum_b align(R + len_b, 128), rounded up to pack_bucket"""
    pack_bucket = check_pack_bucket(pack_bucket)
    Mp = sum(-(-(R + int(v)) // PACK_ALIGN) * PACK_ALIGN for v in lens)
    return Mp if pack_bucket is None else -(-Mp // pack_bucket) * pack_bucket


def pack_plan(lens, R, pack_bucket=None, N=None):
    """lens: ints (list, tuple or CPU int tensor) [B], every one >= 1; R register rows per segment; N: frames per row of the padded
    batch (default max(lens)).  -> PackPlan, every table a CPU tensor:
      seg_start int32 [B]   first packed row of segment b (a multiple of 128)
      seg_klen  int32 [B]   R + len_b: the live rows = the keys of the segment
      tile_seg  int32 [Mp/128]   segment of the 128-row tile, -1 past the last segment
      src_row   int64 [Mp]  b * N + n of the frame held by the packed row, -1 for register and dead rows
      dst_row   int64 [B*N] packed row of frame (b, n), -1 for padding frames
      local_row int64 [Mp]  row index inside the segment's own [R + N] rotary table (registers 0 .. R-1, frame n at R + n), 0 for dead rows
      live_rows = sum_b (R + len_b), dead_rows = Mp - live_rows, padded_rows = B * (R + N)"""
    vals = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    B = len(vals)
    if B < 1 or min(vals) < 1:
        raise ValueError(f"pack_plan: every length must be >= 1, got {vals!r}")
    N = max(vals) if N is None else int(N)
    if max(vals) > N or R < 0:
        raise ValueError(f"pack_plan: lengths {vals!r} do not fit N = {N} (R = {R})")
    Mp = packed_rows(vals, R, pack_bucket)
    seg_start = torch.zeros(B, dtype=torch.int32)
    seg_klen = torch.tensor([R + v for v in vals], dtype=torch.int32)
    tile_seg = torch.full((Mp // PACK_ALIGN,), -1, dtype=torch.int32)
    src_row = torch.full((Mp,), -1, dtype=torch.int64)
    dst_row = torch.full((B * N,), -1, dtype=torch.int64)
    local_row = torch.zeros(Mp, dtype=torch.int64)
    row = 0
    for b, v in enumerate(vals):
        size = -(-(R + v) // PACK_ALIGN) * PACK_ALIGN
        seg_start[b] = row
        tile_seg[row // PACK_ALIGN:(row + size) // PACK_ALIGN] = b
        frames = torch.arange(v)
        src_row[row + R:row + R + v] = b * N + frames
        dst_row[b * N:b * N + v] = row + R + frames
        local_row[row:row + R + v] = torch.arange(R + v)
        row += size
    live = sum(R + v for v in vals)
    return PackPlan(Mp, B, N, R, tuple(vals), seg_start, seg_klen, tile_seg, src_row, dst_row, local_row, live, Mp - live, B * (R + N))


def pack_rows(x, plan, fill=0):
    """x [B, N, ...] -> [1, Mp, ...]: packed row r holds frame src_row[r]; register and dead rows hold `fill`"""
    assert x.shape[0] == plan.B and x.shape[1] == plan.N, (tuple(x.shape), plan.B, plan.N)
    src = plan.src_row.to(x.device)
    flat = x.reshape((plan.B * plan.N,) + tuple(x.shape[2:]))
    out = flat.index_select(0, src.clamp(min=0))
    dead = (src < 0).reshape((-1,) + (1,) * (x.ndim - 2))
    return out.masked_fill(dead, fill).unsqueeze(0)


def unpack_rows(xp, plan):
    """xp [1, Mp, ...] -> [B, N, ...]: frame (b, n) from packed row dst_row[b * N + n]; padding frames hold exactly 0"""
    assert xp.shape[0] == 1 and xp.shape[1] == plan.Mp, (tuple(xp.shape), plan.Mp)
    dst = plan.dst_row.to(xp.device)
    out = xp[0].index_select(0, dst.clamp(min=0))
    pad = (dst < 0).reshape((-1,) + (1,) * (xp.ndim - 2))
    return out.masked_fill(pad, 0).reshape((plan.B, plan.N) + tuple(xp.shape[2:]))


def check_tables(seg_start, seg_klen, tile_seg, Mp, n_seg):
    """What the segment kernels index by: validated on the host before a table reaches the device (include/vbx.h "packed rows")."""
    ss, sk, ts = seg_start.tolist()[:n_seg], seg_klen.tolist()[:n_seg], tile_seg.tolist()
    if Mp % PACK_ALIGN or len(ts) != Mp // PACK_ALIGN:
        raise ValueError(f"packed tables: Mp = {Mp} and {len(ts)} tiles do not agree")
    end = 0
    for s, (a, k) in enumerate(zip(ss, sk)):
        size = -(-k // PACK_ALIGN) * PACK_ALIGN
        if a % PACK_ALIGN or a < end or k < 1 or a + size > Mp:
            raise ValueError(f"packed tables: segment {s} (start {a}, keys {k}) is misaligned, overlaps or leaves Mp = {Mp}")
        if any(t != s for t in ts[a // PACK_ALIGN:(a + size) // PACK_ALIGN]):
            raise ValueError(f"packed tables: tile_seg disagrees with segment {s}")
        end = a + size
    covered = sum(-(-k // PACK_ALIGN) for k in sk)
    if any(t < -1 or t >= n_seg for t in ts) or sum(t >= 0 for t in ts) != covered:
        raise ValueError("packed tables: tile_seg names a segment that does not exist or a tile outside its segment")
