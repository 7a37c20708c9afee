"""Cases, operand builders, fp64 references and metrics of the GEMM edge tests (tests/test_gemm_check_cpu.py checks the checks on the
CPU, tests/test_gemm_edges_gpu.py launches every case).  torch on the CPU only: nothing here touches the library or a device.

Why not `rel_err`: it is one Frobenius norm over the whole result, so a bad tail tile hides under it exactly as attn_check.py describes
for the attention kernels -- one row of an 8200-row bf16 result scaled by 1.01, or one 16-byte store of a ragged column tail left at
zero, passes the 4e-3 bound of tests/test_ops_gpu.py (tests/test_gemm_check_cpu.py asserts that it does).  Here

 * the LINEAR outputs (BF16, F32 and its bf16 copy, the split-K slabs and their reduced sum) are checked per element against fp64 from
   the same rounded operands:  |got - ref| <= u_out |ref| + LINEAR_FACTOR (K + 4) 2^-24 S,  S = (|A| |B|)_ij + |bias_j| + |resid_ij|.
   Any order of a K-term fp32 sum errs by at most (K - 1) 2^-24 times the sum of magnitudes, bias and resid add one rounding each;
   the factor 2 is the margin for the matrix pipe's internal rounding; u_out |ref| is the one rounding to the output type.  The bound
   holds for every element on its own, so a wrong row, a wrong column or one wrong element fails it.  Where it is 0 (an empty split,
   a column of zero weights) the result must be exactly 0;
 * the FUSED outputs (QKV, GEGLU, GELU) are checked per 32 x 64 block -- one gemm5 row block by one head or GEGLU half, a divisor of
   every kernel's tiling -- with the tolerances tests/test_ops_gpu.py states for the whole tensor (BLOCK_TOL), now for the worst block;
 * every operand sits in a larger buffer whose other elements are NaN (the row padding K .. lda, the row after the last, the 16 bytes in
   front of the base), every output in a buffer with one more row and ldc - N more columns filled with a NaN-bit sentinel: afterwards
   the sentinel must be bit-identical and everything inside the extent finite.
"""
import json
import math
import os
import struct
import zlib
from dataclasses import dataclass, replace
from functools import lru_cache

import torch
import torch.nn.functional as F

from attn_check import Checks, worst_tile

# ------------------------------------------------------------------------------------------------ constants
# include/vbx.h (tests/test_gemm_edges_gpu.py asserts that these equal the library's)
NT, NN, TN = 0, 1, 2
EPI_BF16, EPI_F32, EPI_QKV, EPI_GEGLU, EPI_SPLITK, EPI_GELU = 0, 1, 2, 3, 4, 5
GEMM3, GEMM4, GEMM5, BM64, BM128, BM160 = 3, 4, 5, 64, 128, 160
GROUPED = -3  # vbx_gemm_tn_splitk_grouped: gemm3's grouped kernel, no route to ask
KERNEL_NAME = {GEMM3: "gemm3", GEMM4: "gemm4", GEMM5: "gemm5", BM64: "bm64", BM128: "bm128", BM160: "bm160", GROUPED: "grouped"}

# Unit roundoff of round-to-nearest, u = 2^-p for a p-bit significand (hidden bit included): half the spacing of the numbers in [1, 2).
# bf16 has 8 significand bits: u = 2^-8 (an ulp is 2^-7) -- NOT 2^-9; fp16 has 11: 2^-11; fp32 has 24: 2^-24.
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U_ACC = 2.0 ** -24
# margin over the (K - 1) u bound of an fp32 sum for the matrix pipe's internal rounding, per output class.  Worst error / bound measured
# on MI355X over all cases of tests/test_gemm_edges_gpu.py (profiles/gemm_edges_measured.json) in the comment.  (The 16-bit classes sit
# just under 1 by construction: among 10^6 elements one lands half an ulp from its neighbour, which is u_out |ref| itself; the fp32
# classes show how little of the accumulation term the kernels use.)
LINEAR_FACTOR = dict(
    bf16=2,  # 0.993
    f32=2,  # 0.0681
    f32_copy=2,  # 0.994
    slab=2,  # 0.0417
    slab_sum=2,  # 0.0417
)
# tests/test_ops_gpu.py's tolerances of the fused epilogues, here for the worst 32 x 64 block (measured worst block in the comment)
BLOCK_TOL = dict(
    fp16=6e-4,  # 0.000327
    bf16=4e-3,  # 0.00268
    rnorm=1e-5,  # 1.01e-07
)
BLOCK_ROWS, BLOCK_COLS = 32, 64
SPLITK_BK = 64  # k range of a split is a multiple of this in gemm.hip and gemm3.hip: kchunk = ceil(ceil(K / splits) / 64) * 64
Q_PRESCALE = struct.unpack("f", struct.pack("f", 10.0 * math.log2(math.e)))[0]  # any positive fp32 is a valid vbx_gemm_desc.q_prescale
QK_SCALE = 8.0

SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float16: (torch.int16, 0x7E01), torch.float32: (torch.int32, 0x7FC00001)}
_NAN = float("nan")


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    kernel: int  # the kernel this case is meant for: vbx_gemm_route must answer it under `select`
    select: int  # vbx_gemm_select
    mode: int
    epi: int
    M: int
    N: int
    K: int
    f16: bool = False  # fp16 operands
    bias: bool = False
    resid: bool = False
    c2: bool = False  # F32: bf16 copy; GEGLU: bf16 pre-activation
    c3: bool = False  # GEGLU: bf16 copy of C
    train: bool = False  # QKV: qb, kb, v, q_rnorm, k_rnorm
    splits: int = 1
    H: int = 0
    Np: int = 0
    qknorm: bool = True
    strided: bool = False  # lda / ldb / ldc above the row length, padding poisoned
    cu_limit: int = 0  # gemm5: 0 no limit, 1 vbx_gemm5_cu_limit(panels), 2 vbx_gemm5_cu_limit(panels + 1)

    @property
    def name(self):
        e = {EPI_BF16: "bf16", EPI_F32: "f32", EPI_QKV: "qkv", EPI_GEGLU: "geglu", EPI_SPLITK: "splitk", EPI_GELU: "gelu"}[self.epi]
        flags = "".join(f for f, on in (("h", self.f16), ("b", self.bias), ("r", self.resid), ("2", self.c2), ("3", self.c3), ("t", self.train),
                                        ("n", self.epi == EPI_QKV and not self.qknorm)) if on)
        s = f"{KERNEL_NAME[self.kernel]}-s{self.select}-{('nt', 'nn', 'tn')[self.mode]}-{e}{'-' + flags if flags else ''}-{self.M}x{self.N}x{self.K}"
        if self.epi == EPI_SPLITK:
            s += f"-sp{self.splits}"
        if self.cu_limit:
            s += f"-cu{self.cu_limit}"
        return s + ("-strided" if self.strided else "-dense")

    @property
    def panels(self):  # gemm5: 256-feature weight panels
        return -(-(-(-self.N // 64)) // 4)

    def key(self):  # what the logical operands and the reference depend on
        return (self.mode, self.epi, self.M, self.N, self.K, self.f16, self.bias, self.resid, self.c2, self.c3, self.train, self.splits,
                self.H, self.Np, self.qknorm)


def _both(cases):
    return [replace(c, strided=s) for c in cases for s in (False, True)]


def _linear(kernel, select, shapes_nt, shapes_nn):
    """The light epilogues on one kernel: bf16 with and without bias, fp32 with every optional pointer and with none, fp16 operands."""
    out = []
    for i, (M, N, K) in enumerate(shapes_nt):
        out.append(Case(kernel, select, NT, EPI_BF16, M, N, K, bias=i % 2 == 0))
        out.append(Case(kernel, select, NT, EPI_F32, M, N, K, bias=True, resid=True, c2=True) if i % 2 == 0 else
                   Case(kernel, select, NT, EPI_F32, M, N, K, f16=True, resid=i % 4 == 1))
    for i, (M, N, K) in enumerate(shapes_nn):
        out.append(Case(kernel, select, NN, EPI_BF16, M, N, K, bias=i % 2 == 1))
        out.append(Case(kernel, select, NN, EPI_F32, M, N, K, bias=i % 2 == 0, c2=i % 2 == 0))
    return out


def _fused(kernel, select, M, K, H, Np, n_geglu, n_gelu):
    """QKV (training and inference form), GEGLU (bf16 operands with the pre-activation; fp16 operands, training and inference) and
    GELU where the kernel has it."""
    out = [Case(kernel, select, NT, EPI_QKV, M, 3 * H * 64, K, f16=True, train=True, H=H, Np=Np),
           Case(kernel, select, NT, EPI_QKV, M, 3 * H * 64, K, f16=True, train=False, H=H, Np=Np, qknorm=False),
           Case(kernel, select, NT, EPI_GEGLU, M, n_geglu, K, bias=True, c2=True),
           Case(kernel, select, NT, EPI_GEGLU, M, n_geglu, K, f16=True, bias=True, c2=True, c3=True),
           Case(kernel, select, NT, EPI_GEGLU, M, n_geglu, K, f16=True, bias=True)]
    if n_gelu:
        out.append(Case(kernel, select, NT, EPI_GELU, M, n_gelu, K, f16=True, bias=True))
    return out


def _table():
    """Per kernel, at that kernel's own constants (BM 64 / 128 / 160 / 256 / 128, gemm5's 32-row blocks; BN 128 / 256; BK 32 / 64):
    M in {1, tile - 1, tile + 1}, N in {8, one tile + 8}, K in {8, BK - 8, BK + 8}, odd K and K < BK for TN.  The shapes that reach a
    128-wide tile without a big matrix follow gemm_route.hpp's tile128_family(); the GPU test asserts the route of every case."""
    t = []
    # 64 x 128 (BK 32): anything small
    t += _linear(BM64, 0, [(65, 136, 72), (1, 8, 8), (63, 136, 24), (129, 8, 40)], [(65, 136, 72), (1, 8, 8), (63, 136, 24), (129, 8, 40)])
    t += _fused(BM64, 1, 65, 72, 2, 13, 256, 136)
    # 128 x 128 (BK 32), NT: K just above 1024
    t += _linear(BM128, 0, [(129, 136, 1032), (127, 8, 1048), (1, 136, 1064)], [])
    t += _fused(BM128, 1, 129, 1032, 2, 43, 256, 136)
    # 128 x 128, NN: 3 x 129 = 387 tiles, a 44-row tail and an 8-column tail
    t += _linear(BM128, 0, [], [(300, 16392, 72)])
    # 128 x 128, TN split-K (vbx_gemm sends every TN here unless gemm3 is selected): odd K, K < BK, ragged M and N, an empty split
    for sel in (0, 1):
        t += [Case(BM128, sel, TN, EPI_SPLITK, M, N, K, splits=sp) for M, N, K, sp in
              ((136, 136, 72, 3), (264, 200, 33, 1), (8, 8, 40, 2), (136, 264, 133, 2), (8, 136, 7, 1))]
    # select 1: the training form of to_qkv at K = 512 on the 128-wide kernels (what VBX_GEMM5=0 runs), and the bf16 product gemm5 takes
    t += [Case(BM64, 1, NT, EPI_QKV, 100, 384, 512, f16=True, train=True, H=2, Np=25),
          Case(BM64, 1, NT, EPI_BF16, 100, 576, 512)]
    # 160 x 128 (BK 64), one round: 96 .. 256 tiles
    t += _linear(BM160, 0, [(161, 6152, 72), (159, 12296, 56), (1, 12296, 8)], [(161, 6152, 72), (159, 12296, 56)])
    t += _fused(BM160, 1, 161, 72, 32, 23, 6144, 6152)
    # 160 x 128, the multi-round arm: light epilogue, K >= 1024, 2 x 130 = 260 tiles
    t += [Case(BM160, 0, NT, EPI_BF16, 161, 16520, 1032, bias=True)]
    # 256 x 256 (BK 64, select 2) and 128 x 256 (BK 32, select 3)
    t += _linear(GEMM3, 2, [(65, 136, 72), (255, 264, 56), (257, 8, 8), (1, 264, 72)], [(65, 136, 72), (255, 264, 56), (257, 8, 8)])
    t += _fused(GEMM3, 2, 65, 72, 2, 13, 384, 0)
    t += [Case(GEMM3, 2, TN, EPI_SPLITK, M, N, K, splits=sp) for M, N, K, sp in ((136, 136, 72, 3), (264, 264, 56, 1), (8, 8, 40, 2))]
    t += _linear(GEMM4, 3, [(65, 136, 72), (127, 264, 24), (129, 8, 8), (1, 264, 40)], [(65, 136, 72), (127, 264, 24), (129, 8, 40)])
    t += _fused(GEMM4, 3, 65, 72, 2, 13, 384, 0)
    t = _both(t)
    # gemm5 (auto, K = 512): N = 576 leaves three idle waves in the last panel (GEGLU needs N % 128 == 0: 640, two idle waves)
    g5 = []
    for M, Np in ((1, 1), (31, 31), (32, 16), (33, 11), (100, 25), (2017, 2017)):
        for lim in (0, 1, 2):
            if lim and M == 2017 or lim == 2 and M < 33:
                continue
            for s in ((False, True) if lim == 0 and M != 2017 else (True,)):
                g5 += [Case(GEMM5, 0, NT, EPI_QKV, M, 576, 512, f16=True, train=True, H=3, Np=Np, strided=s, cu_limit=lim),
                       Case(GEMM5, 0, NT, EPI_QKV, M, 576, 512, f16=True, train=False, H=3, Np=Np, strided=s, cu_limit=lim, qknorm=M % 2 == 1),
                       Case(GEMM5, 0, NT, EPI_GEGLU, M, 640, 512, f16=True, bias=True, c2=True, c3=True, strided=s, cu_limit=lim),
                       Case(GEMM5, 0, NT, EPI_GEGLU, M, 640, 512, f16=True, bias=True, strided=s, cu_limit=lim),
                       Case(GEMM5, 0, NT, EPI_BF16, M, 576, 512, strided=s, cu_limit=lim)]
    return t + g5


CASES = _table()
# vbx_gemm_tn_splitk_grouped with the first n of these jobs, n = 1 .. 4: odd K, K = 40, M = N = 8, an empty split
GROUPED_JOBS = [Case(GROUPED, 0, TN, EPI_SPLITK, M, N, K, splits=sp) for M, N, K, sp in ((8, 8, 40, 3), (136, 264, 133, 2), (264, 136, 33, 1), (264, 264, 72, 3))]


# ------------------------------------------------------------------------------------------------ operands and references
def _dt16(case):
    return torch.float16 if case.f16 else torch.bfloat16


def geglu_fd(case):
    """Features per GEGLU half that carry weights; the other N / 2 - fd are the packing's padding (zero weights, zero bias)."""
    return case.N // 2 - 21


def rot_tables(Np):
    from oracle import restate

    R = min(16, Np // 2)  # register tokens in front, as the model lays a sequence out
    pos = torch.cat((torch.full((R,), -10000, dtype=torch.long), torch.arange(Np - R)))
    fr = restate.rotary_freqs(pos, 64, 50000.0)
    return fr, fr[:, :32].cos().contiguous(), fr[:, :32].sin().contiguous()


@lru_cache(maxsize=6)
def _logical(key):
    """Seeded logical operands of a case, rounded to their types (shared by its dense / strided / select / cu_limit variants)."""
    mode, epi, M, N, K, f16, bias, resid, c2, c3, train, splits, H, Np, qknorm = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    dt = torch.float16 if f16 else torch.bfloat16
    a_shape = (K, M) if mode == TN else (M, K)
    b_shape = (N, K) if mode == NT else (K, N)
    ops = {"A": torch.randn(a_shape, generator=g).to(dt), "B": (torch.randn(b_shape, generator=g) * K ** -0.5).to(dt)}
    if bias:
        ops["bias"] = torch.randn(N, generator=g)
    if resid:
        ops["resid"] = torch.randn(M, N, generator=g)
    if epi == EPI_GEGLU:  # interleaved packing: 128-row blocks of 64 value rows | 64 gate rows; features >= fd are padding
        fd = N // 2 - 21
        f = (torch.arange(N) // 128) * 64 + torch.arange(N) % 64
        ops["B"][f >= fd] = 0
        ops["bias"] = ops["bias"] * 0.1
        ops["bias"][f >= fd] = 0
    if epi == EPI_QKV:
        ops["q_gamma"] = 1 + 0.1 * torch.randn(H, 64, generator=g)
        ops["k_gamma"] = 1 + 0.1 * torch.randn(H, 64, generator=g)
        ops["fr"], ops["rot_cos"], ops["rot_sin"] = rot_tables(Np)
    return ops


def split_ranges(K, splits):
    kchunk = -(-(-(-K // splits)) // SPLITK_BK) * SPLITK_BK
    return [(min(K, s * kchunk), min(K, (s + 1) * kchunk)) for s in range(splits)]


def _heads(x, Bsz, Np, H):  # [M, H * 64] -> the kernels' [B, H, Np, 64], as rows of 64
    return x.reshape(Bsz, Np, H, 64).permute(0, 2, 1, 3).reshape(Bsz * H * Np, 64)


def _forward(case, ops, dt):
    """Every output of the case from the rounded operands, computed in `dt` (float64: the reference; float32: the stand-in), as
    {name: [rows, cols]} in the output buffer's own layout."""
    from oracle import restate

    A, B = ops["A"].to(dt), ops["B"].to(dt)
    M, N, K = case.M, case.N, case.K
    if case.epi == EPI_SPLITK:
        slabs = [A[kb:ke].t() @ B[kb:ke] if ke > kb else torch.zeros(M, N, dtype=dt) for kb, ke in split_ranges(K, case.splits)]
        slabs = torch.stack(slabs)
        return {"slabs": slabs.reshape(case.splits * M, N), "sum": slabs.sum(0)}
    acc = A @ B.t() if case.mode == NT else A @ B
    if case.bias:
        acc = acc + ops["bias"].to(dt)
    if case.epi == EPI_BF16:
        return {"C": acc}
    if case.epi == EPI_F32:
        if case.resid:
            acc = acc + ops["resid"].to(dt)
        return {"C": acc, "C2": acc} if case.c2 else {"C": acc}
    if case.epi == EPI_GELU:
        return {"C": F.gelu(acc)}
    if case.epi == EPI_GEGLU:
        hv = acc.view(M, N // 128, 2, 64)
        out = F.gelu(hv[:, :, 1]).reshape(M, N // 2) * hv[:, :, 0].reshape(M, N // 2)
        res = {"C": out}
        if case.c2:
            res["C2"] = acc
        if case.c3:
            res["C3"] = out
        return res
    Bsz, Np, H = M // case.Np, case.Np, case.H
    qkv = acc.view(M, 3, H, 64)
    q, k, v = (qkv[:, i].reshape(Bsz, Np, H, 64).permute(0, 2, 1, 3) for i in range(3))  # [B, H, Np, 64]
    res = {}
    if case.train:
        res["q_rnorm"] = (1 / q.norm(dim=-1)).reshape(-1, 1)
        res["k_rnorm"] = (1 / k.norm(dim=-1)).reshape(-1, 1)
    if case.qknorm:
        q = restate.l2norm_scale(q, 64) * ops["q_gamma"].to(dt)[:, None, :]
        k = restate.l2norm_scale(k, 64) * ops["k_gamma"].to(dt)[:, None, :]
    fr = ops["fr"].to(dt)
    q, k = restate.apply_rotary(fr, q), restate.apply_rotary(fr, k)
    res.update(q16=(q * Q_PRESCALE).reshape(-1, 64), k16=k.reshape(-1, 64), v16=v.reshape(-1, 64))
    if case.train:
        res.update(qb=q.reshape(-1, 64), kb=k.reshape(-1, 64), v=v.reshape(-1, 64))
    return res


def out_dtypes(case):
    d16 = _dt16(case)
    return {EPI_BF16: {"C": torch.bfloat16},
            EPI_F32: {"C": torch.float32, "C2": torch.bfloat16},
            EPI_GELU: {"C": torch.float16},
            EPI_GEGLU: {"C": d16, "C2": torch.bfloat16, "C3": torch.bfloat16},
            EPI_SPLITK: {"slabs": torch.float32, "sum": torch.float32},
            EPI_QKV: {"q16": torch.float16, "k16": torch.float16, "v16": torch.float16, "qb": torch.bfloat16, "kb": torch.bfloat16,
                      "v": torch.bfloat16, "q_rnorm": torch.float32, "k_rnorm": torch.float32}}[case.epi]


@lru_cache(maxsize=6)
def _reference(key, case):
    ops = _logical(key)
    ref = _forward(case, ops, torch.float64)
    S = None
    if case.epi in (EPI_BF16, EPI_F32, EPI_SPLITK):  # sum of magnitudes of everything added into an element
        A, B = ops["A"].double().abs(), ops["B"].double().abs()
        if case.epi == EPI_SPLITK:
            s = torch.stack([A[kb:ke].t() @ B[kb:ke] if ke > kb else torch.zeros(case.M, case.N, dtype=torch.float64)
                             for kb, ke in split_ranges(case.K, case.splits)])
            S = {"slabs": s.reshape(case.splits * case.M, case.N), "sum": s.sum(0)}
        else:
            s = A @ B.t() if case.mode == NT else A @ B
            if case.bias:
                s = s + ops["bias"].double().abs()
            if case.resid:
                s = s + ops["resid"].double().abs()
            S = {"C": s, "C2": s}
    return ref, S


def reference(case):
    """({name: fp64 reference [rows, cols]}, {name: S} for the linear outputs or None)."""
    base = replace(case, kernel=0, select=0, strided=False, cu_limit=0)
    return _reference(case.key(), base)


def standin(case):
    """What a correct kernel may answer: a torch fp32 product of the exactly converted operands through the epilogue in fp32, rounded
    once to the output type.  {name: [rows, cols] in the output type}."""
    out = _forward(case, _logical(case.key()), torch.float32)
    dts = out_dtypes(case)
    res = {n: x.to(dts[n]) for n, x in out.items()}
    if "C2" in res and case.epi == EPI_F32:
        res["C2"] = res["C"].to(torch.bfloat16)
    return res


# ------------------------------------------------------------------------------------------------ buffers
@dataclass
class OutSpec:
    dtype: torch.dtype
    rows: int
    cols: int
    ld: int

    def new(self):  # one extra row, ld - cols extra columns, the sentinel everywhere
        it, val = SENTINEL[self.dtype]
        return torch.full(((self.rows + 1) * self.ld,), val, dtype=it).view(self.dtype)

    def view(self, buf):
        return buf[: self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols]

    def outside(self, buf):  # the raw bits of everything outside the extent
        it, _ = SENTINEL[self.dtype]
        m = torch.ones((self.rows + 1) * self.ld, dtype=torch.bool)
        m[: self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols] = False
        return buf.view(it)[m]


def _embed(x, ld):
    """x [rows, cols] inside a NaN-filled buffer: 16 bytes in front of the base, row padding cols .. ld, one more row behind.
    Returns (flat buffer, element offset of the base)."""
    rows, cols = x.shape
    front = 16 // x.element_size()
    buf = torch.full((front + (rows + 1) * ld,), _NAN, dtype=x.dtype)
    buf[front: front + rows * ld].view(rows, ld)[:, :cols] = x
    return buf, front


@dataclass
class Built:
    case: Case
    inputs: dict  # name -> (flat buffer, element offset of the base)
    outs: dict  # name -> OutSpec
    scal: dict  # vbx_gemm_desc's integer / float fields
    ptrs: dict  # vbx_gemm_desc pointer field -> ("in" | "out", name)


def build(case):
    ops = _logical(case.key())
    M, N, K = case.M, case.N, case.K
    pad, cpad = (24, 8) if case.strided else (0, 0)
    lda, ldb = ops["A"].shape[1] + pad, ops["B"].shape[1] + pad
    inputs = {"A": _embed(ops["A"], lda), "B": _embed(ops["B"], ldb)}
    scal = dict(mode=case.mode, epilogue=case.epi, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=0, splits=case.splits, f16=int(case.f16))
    ptrs = {"A": ("in", "A"), "B": ("in", "B")}
    outs = {}
    dts = out_dtypes(case)
    if case.bias:
        inputs["bias"] = _embed(ops["bias"][None], N)
        ptrs["bias"] = ("in", "bias")
    if case.epi in (EPI_BF16, EPI_F32, EPI_GELU):
        ldc = scal["ldc"] = N + cpad
        outs["C"] = OutSpec(dts["C"], M, N, ldc)
        if case.resid:
            inputs["resid"] = _embed(ops["resid"], ldc)
            ptrs["resid"] = ("in", "resid")
        if case.c2:
            outs["C2"] = OutSpec(dts["C2"], M, N, ldc)
    elif case.epi == EPI_GEGLU:
        ldc = scal["ldc"] = N // 2 + cpad
        outs["C"] = OutSpec(dts["C"], M, N // 2, ldc)
        if case.c2:
            outs["C2"] = OutSpec(dts["C2"], M, N, N)
        if case.c3:
            outs["C3"] = OutSpec(dts["C3"], M, N // 2, ldc)
    elif case.epi == EPI_SPLITK:
        outs["slabs"] = OutSpec(torch.float32, case.splits * M, N, N)
        outs["sum"] = OutSpec(torch.float32, M, N, N + cpad)  # vbx_splitk_reduce's destination
    else:
        rows = M * case.H
        scal.update(Np=case.Np, H=case.H, qk_scale=QK_SCALE if case.qknorm else 0.0, q_prescale=Q_PRESCALE)
        for n in ("q_gamma", "k_gamma", "rot_cos", "rot_sin"):
            inputs[n] = _embed(ops[n].reshape(1, -1), ops[n].numel())
            ptrs[n] = ("in", n)
        for n in ("q16", "k16", "v16") + (("qb", "kb", "v", "q_rnorm", "k_rnorm") if case.train else ()):
            outs[n] = OutSpec(dts[n], rows, 1 if n.endswith("rnorm") else 64, 1 if n.endswith("rnorm") else 64)
    for n in outs:
        if n not in ("slabs", "sum"):
            ptrs[n] = ("out", n)
    if case.epi == EPI_SPLITK:
        ptrs["C"] = ("out", "slabs")
    return Built(case, inputs, outs, scal, ptrs)


def fill(built, logical):
    """Output buffers as a launch leaves them, from {name: [rows, cols]} results: the extent written, the sentinel elsewhere."""
    res = {}
    for n, spec in built.outs.items():
        res[n] = spec.new()
        spec.view(res[n])[:] = logical[n]
    return res


# ------------------------------------------------------------------------------------------------ metrics
def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def linear_ratios(got, ref, S, K, u_out, factor):
    """|got - ref| / (u_out |ref| + factor (K + 4) 2^-24 S) per element; where the bound is 0 the result must be exactly 0 (ratio 0,
    inf otherwise).  NaN propagates."""
    got, ref = got.detach().double().cpu(), ref.double()
    err = (got - ref).abs()
    bound = u_out * ref.abs() + factor * (K + 4) * U_ACC * S
    ratio = err / bound.clamp(min=1e-300)
    ratio = torch.where(bound == 0, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)), ratio)
    return torch.where(torch.isnan(err), torch.full_like(err, math.nan), ratio)


def block_errors(got, ref, rows=BLOCK_ROWS, cols=BLOCK_COLS, floor=1e-3):
    """tile_errors in two dimensions: the relative error of every `rows` x `cols` block of a matrix, [ceil(R / rows), ceil(C / cols)].
    A block's error is ||got - ref|| / max(||ref||, floor * rms(ref) * sqrt(elements of the block)); a block whose reference is exactly
    zero must be exactly zero (error 0 if it is, inf otherwise); NaN propagates."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and ref.dim() == 2, (got.shape, ref.shape)
    R, C = ref.shape
    nr, nc = -(-R // rows), -(-C // cols)

    def blocks(x):
        x = F.pad(x, (0, nc * cols - C, 0, nr * rows - R))
        return x.view(nr, rows, nc, cols).permute(0, 2, 1, 3).reshape(nr, nc, rows * cols)

    r, d, gt = blocks(ref), blocks(got - ref), blocks(got)
    br = torch.full((nr,), float(rows))
    br[-1] = R - (nr - 1) * rows
    bc = torch.full((nc,), float(cols))
    bc[-1] = C - (nc - 1) * cols
    rms = float(ref.norm()) / math.sqrt(max(ref.numel(), 1))
    fl = floor * rms * torch.sqrt(br[:, None] * bc[None, :]).double()
    rn, dn = r.norm(dim=-1), d.norm(dim=-1)
    err = dn / torch.maximum(rn, fl).clamp(min=1e-300)
    gz = gt.abs().amax(dim=-1)
    err = torch.where(rn == 0, torch.where(gz == 0, torch.zeros_like(err), torch.full_like(err, math.inf)), err)
    return torch.where(torch.isnan(dn) | torch.isnan(gz), torch.full_like(err, math.nan), err)


class GemmChecks(Checks):
    """attn_check.Checks with the log of these tests: GEMM_CHECK_LOG=<file> appends one JSON line per case with every measured value
    (how profiles/gemm_edges_measured.json and the figures beside LINEAR_FACTOR / BLOCK_TOL were made)."""

    def done(self):
        if os.environ.get("GEMM_CHECK_LOG"):
            with open(os.environ["GEMM_CHECK_LOG"], "a") as f:
                f.write(json.dumps({"case": self.case, "values": [(n, v if isinstance(v, bool) else float(v), b) for n, v, b in self.seen]}) + "\n")
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)


def _to2d(case, name, x):
    """A fused output as the matrix whose 32 x 64 blocks are a row block by a head / GEGLU half / rnorm column."""
    if case.epi != EPI_QKV:
        return x
    Bsz, Np, H = case.M // case.Np, case.Np, case.H
    w = x.shape[1]
    return x.reshape(Bsz, H, Np, w).permute(0, 2, 1, 3).reshape(case.M, H * w)


def linear_class(case, name):
    if case.epi == EPI_SPLITK:
        return "slab" if name == "slabs" else "slab_sum"
    return "bf16" if case.epi == EPI_BF16 else "f32" if name == "C" else "f32_copy"


def check(built, results, label=None):
    """Every bound of one case on {name: flat output buffer} (on the CPU, as build / fill lay them out); one failure lists them all."""
    case = built.case
    ck = GemmChecks(label or case.name)
    ref, S = reference(case)
    for n, spec in built.outs.items():
        buf = results[n].cpu()
        it, val = SENTINEL[spec.dtype]
        ck.true(f"{n} sentinel (rows past M, columns past N) untouched", bool((spec.outside(buf) == val).all()))
        got = spec.view(buf)
        ck.true(f"{n} finite inside the extent", bool(torch.isfinite(got.float()).all()))
        if S is not None:
            cls = linear_class(case, n)
            r = linear_ratios(got, ref[n], S[n], case.K, U_OUT[spec.dtype], LINEAR_FACTOR[cls])
            w, idx = worst_tile(r)
            ck.le(f"{n} [{cls}] error / bound at {idx}", w, 1.0)
        else:
            cls = "rnorm" if n.endswith("rnorm") else "fp16" if spec.dtype == torch.float16 else "bf16"
            e = block_errors(_to2d(case, n, got), _to2d(case, n, ref[n]))
            w, idx = worst_tile(e)
            ck.le(f"{n} [{cls}] block{idx}", w, BLOCK_TOL[cls])
            if case.epi == EPI_GEGLU and n in ("C", "C3"):
                ck.true(f"{n} padding columns exactly zero", bool((got[:, geglu_fd(case):].float() == 0).all()))
    ck.done()
