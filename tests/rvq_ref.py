"""The residual vector quantizer of csrc/rvq.hip restated on the CPU, and the checker of its search contract.  The libraries whose
arithmetic this follows (vector_quantize_pytorch's ResidualVQ with Euclidean codebooks as EnCodec uses it, Vocos's
codes_to_features) are absent, so parity with them is UNPINNED; the kernels are tested against this file.

Per frame, r_0 = x and for q = 0 .. Q-1:  code_q = argmin_k d(k),  d(k) = |c_qk|^2 - 2 r_q . c_qk  (= |r_q - c_qk|^2 - |r_q|^2),
the lowest index on an exact tie;  r_{q+1} = r_q - c_q[code_q];  quantized = c_0[code_0] + c_1[code_1] + ...

THE SEARCH CONTRACT, checked teacher-forced (check_search).  Once one code differs from another search's, every later residual
legitimately differs, so code sequences are never compared.  For each stage the checker rebuilds r_q in fp64 from the inputs and
the search's OWN earlier codes and requires

    d(code_q) - min_k d(k)  <=  BOUND = (D + 2) * 2^-23 * (|r_q| + max_k |c_qk|)^2          (d in fp64)

Derivation: an fp32 dot product of length D, in any order, errs by at most D 2^-24 |r| |c| (it enters d doubled); an fp32 table
of |c|^2 errs by at most (D + 1) 2^-24 |c|^2 (D products, D - 1 additions); forming d rounds once more, 2^-24 |d| with |d| <=
(|r| + |c|)^2; that is at most (D + 2) 2^-24 (|r| + |c|)^2 per candidate, and two candidates are compared.  (The residual the
kernel carries is fp32 while the rebuilt one is fp64: Q - 1 subtractions, each within 2^-24 of a value no larger than |r| + |c|
per component -- covered by the same slack only loosely, so the GPU test inputs keep Q <= 8 and the fp32 restatement below is
itself held to the bound on every one of them, tests/test_rvq_cpu.py.)  Wherever the fp64 gap between the best and the second
best candidate exceeds BOUND the code must therefore BE the fp64 argmin: check_search counts those stages too ("forced")."""
import torch

U23 = 2.0 ** -23


def random_case(M, D, K, Q, seed, scale=1.0):
    """frames [M, D] and codebooks [Q, K, D] as an RVQ sees them: later codebooks are smaller, frames lie near sums of codewords"""
    g = torch.Generator().manual_seed(seed)
    cb = torch.stack([torch.randn(K, D, generator=g) * scale * 0.6 ** q for q in range(Q)])
    x = torch.zeros(M, D)
    for q in range(Q):
        x += cb[q][torch.randint(0, K, (M,), generator=g)]
    return x + 0.1 * scale * torch.randn(M, D, generator=g), cb


def planted(M, D, K, seed):
    """One-stage inputs on which a search of less than fp32 class fails the contract: codewords in pairs c_{2j+1} = c_{2j} + 1e-2
    u_j (u_j a unit vector), frames x = c_{2j} + n with n about 0.05 per component across u_j and the component along u_j set so
    that the fp64 gap d(2j + 1) - d(2j) = eps^2 - 2 eps (n . u_j) is a seeded multiple in [1.5, 6] of BOUND, of random sign.
    Returns (x [M, D], codebooks [1, K, D])."""
    assert K % 2 == 0
    g = torch.Generator().manual_seed(seed)
    eps = 1e-2
    base = torch.randn(K // 2, D, generator=g, dtype=torch.float64)
    u = torch.randn(K // 2, D, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    cb = torch.stack((base, base + eps * u), dim=1).reshape(K, D).float()  # the fp32 table is the input from here on
    c64 = cb.double()
    cmax = float(c64.norm(dim=1).max())
    j = torch.randint(0, K // 2, (M,), generator=g)
    lo, hi = c64[2 * j], c64[2 * j + 1]
    du = hi - lo  # eps * u as the fp32 table holds it
    e = du.norm(dim=1)
    uu = du / e[:, None]
    n = 0.05 * torch.randn(M, D, generator=g, dtype=torch.float64)
    n = n - (n * uu).sum(1, keepdim=True) * uu
    mult = (1.5 + 4.5 * torch.rand(M, generator=g, dtype=torch.float64)) * (2.0 * torch.randint(0, 2, (M,), generator=g) - 1.0)
    a = torch.zeros(M, dtype=torch.float64)
    for _ in range(4):  # BOUND depends on |x|, hence (weakly) on a: a few fixed-point passes
        x = lo + n + a[:, None] * uu
        bound = (D + 2) * U23 * (x.norm(dim=1) + cmax) ** 2
        # d(hi) - d(lo) = |hi|^2 - |lo|^2 - 2 x . du,  x . du = lo . du + a e
        a = ((hi.pow(2).sum(1) - lo.pow(2).sum(1) - mult * bound) / 2.0 - (lo * du).sum(1)) / e
    return (lo + n + a[:, None] * uu).float(), cb[None]


def distances64(r, c):
    """d(k) = |c_k|^2 - 2 r . c_k in fp64: r [M, D], c [K, D] -> [M, K]"""
    return c.pow(2).sum(1)[None, :] - 2.0 * r @ c.t()


def check_search(x, cb, codes):
    """x [M, D] fp32, cb [Q, K, D] fp32, codes int64 [M, Q] -> dict(violations, worst (largest regret / BOUND), forced (stages whose
    fp64 gap exceeds BOUND), forced_wrong (of those, codes that are not the fp64 argmin))"""
    x64, c64, codes = x.double(), cb.double(), codes.cpu()
    M, D = x64.shape
    Q, K, _ = c64.shape
    assert codes.shape == (M, Q) and codes.dtype == torch.int64 and int(codes.min()) >= 0 and int(codes.max()) < K
    r = x64.clone()
    out = dict(violations=0, worst=0.0, forced=0, forced_wrong=0)
    rows = torch.arange(M)
    for q in range(Q):
        d = distances64(r, c64[q])
        bound = (D + 2) * U23 * (r.norm(dim=1) + c64[q].norm(dim=1).max()) ** 2
        two = torch.topk(d, 2, dim=1, largest=False).values
        regret = d[rows, codes[:, q]] - two[:, 0]
        out["violations"] += int((regret > bound).sum())
        out["worst"] = max(out["worst"], float((regret / bound).max()))
        forced = (two[:, 1] - two[:, 0]) > bound
        out["forced"] += int(forced.sum())
        out["forced_wrong"] += int((forced & (codes[:, q] != d.argmin(dim=1))).sum())
        r = r - c64[q][codes[:, q]]
    return out


def split3(t, dtype, shift=8):
    """hi + lo parts of fp32 values in a 16-bit format (lo scaled by 2^shift while it is rounded, as csrc/precise.hip keeps small lo
    parts out of the subnormals)"""
    hi = t.to(dtype).float()
    lo = ((t - hi) * 2.0 ** shift).to(dtype).float() * 2.0 ** -shift
    return hi, lo


def search(x, cb, mode="fp32"):
    """The search written with torch on the CPU, the residual carried in fp32 as on the device.  mode: "fp32" (the restatement the
    kernels are compared with), "fp16x3" / "bf16x3" (hi/lo-split 16-bit operands, the lo . lo product dropped, fp32 accumulation),
    "fp16" (ONE rounding of both operands to fp16: NOT fp32 class).  Returns (codes [M, Q], quantized [M, D])."""
    Q = cb.shape[0]
    r = x.float().clone()
    codes, quant = [], None
    for q in range(Q):
        c = cb[q].float()
        norms = c.pow(2).sum(1)
        if mode == "fp32":
            dots = r @ c.t()
        elif mode == "fp16":
            dots = r.half().float() @ c.half().float().t()
        else:
            dt = torch.float16 if mode == "fp16x3" else torch.bfloat16
            (rh, rl), (ch, cl) = split3(r, dt), split3(c, dt)
            dots = rh @ ch.t() + (rh @ cl.t() + rl @ ch.t())
        d = norms[None, :] - 2.0 * dots
        k = d.argmin(dim=1)  # the first of equal minima
        sel = c[k]
        codes.append(k)
        quant = sel.clone() if quant is None else quant + sel
        r = r - sel
    return torch.stack(codes, dim=1), quant


def gather_sum(codes, cb):
    """the fp32 loop acc = c_0[code_0]; acc = acc + c_q[code_q]: codes int64 [M, Q'], cb [Q, K, D] -> [M, D]; an index outside
    [0, K) contributes zero"""
    K = cb.shape[1]
    acc = torch.zeros(codes.shape[0], cb.shape[2], dtype=torch.float32)
    for q in range(codes.shape[1]):
        k = codes[:, q]
        ok = (k >= 0) & (k < K)
        acc = acc + cb[q].float()[k.clamp(0, K - 1)] * ok[:, None].float()
    return acc


# (name, B, N, D, K, Q): the shapes of tests/test_rvq_gpu.py, the smallest at which the kernel can go wrong -- one frame of the
# narrowest width; a frame tail over several batch elements; K that is a multiple of no chunk (the padded codewords must never
# win); the published widths over more than one tile and two batch elements; and one width per chunk size of the kernel above
# D = 128, where fewer waves multiply: D 136 and 248 stream chunks of 64 codewords whose float4 count (16 D) is no multiple of the
# 256 loading threads, with K a multiple of the chunk (the last fetch of the last stage ends at the end of the table) and not;
# D 256 streams chunks of 32 (one multiplying wave)
CASES = [("one", 1, 1, 8, 2, 1), ("tail", 7, 11, 32, 64, 4), ("k1000", 1, 33, 128, 1000, 3), ("published", 2, 150, 128, 1024, 8),
         ("d136", 2, 35, 136, 192, 2), ("d248", 1, 70, 248, 100, 2), ("d256", 1, 70, 256, 96, 2)]
PLANTED = [("planted-32", 256, 32, 64), ("planted-128", 256, 128, 1024)]  # (name, M, D, K), one stage


def case_inputs(name):
    for i, (n, B, N, D, K, Q) in enumerate(CASES):
        if n == name:
            x, cb = random_case(B * N, D, K, Q, seed=100 + i)
            return x.reshape(B, N, D), cb
    for i, (n, M, D, K) in enumerate(PLANTED):
        if n == name:
            x, cb = planted(M, D, K, seed=200 + i)
            return x.reshape(1, M, D), cb
    raise KeyError(name)


TIE_PAIRS = ((3, 40), (0, 63))


def tie_case(seed=7):
    """K = 64, two stages, stage-0 codewords 40 and 63 exact copies of 3 and 0; 40 frames next to each of the four indices and 40
    elsewhere.  Returns (x [1, 200, 32], cb [2, 64, 32], lower index expected at stage 0 or -1 [200])."""
    g = torch.Generator().manual_seed(seed)
    cb = torch.stack((torch.randn(64, 32, generator=g), 0.5 * torch.randn(64, 32, generator=g)))
    for lo, hi in TIE_PAIRS:
        cb[0, hi] = cb[0, lo]
    near = torch.tensor([3] * 40 + [40] * 40 + [0] * 40 + [63] * 40 + [17] * 40)
    x = cb[0, near] + 0.05 * torch.randn(200, 32, generator=g)
    expect = torch.tensor([3] * 80 + [0] * 80 + [-1] * 40)
    return x[None], cb, expect


def exact_case(seed=9):
    """frames EXACTLY equal to stage-0 codewords: zero residual, so stage 1 sees d(k) = |c_1k|^2 and must return the lowest index of
    the smallest -- codeword 5 of stage 1 is by far the shortest and codeword 20 is its exact copy.  Returns (x [1, 64, 32], cb
    [2, 64, 32], the stage-0 codes)."""
    g = torch.Generator().manual_seed(seed)
    cb = torch.stack((torch.randn(64, 32, generator=g), 0.5 * torch.randn(64, 32, generator=g)))
    cb[1, 5] *= 0.01
    cb[1, 20] = cb[1, 5]
    k0 = torch.randperm(64, generator=g)
    return cb[0, k0].clone()[None], cb, k0
