"""fp64 restatement of the aligner primitives (voicebox_pytorch_amd.maximum_path / forward_sum_loss; csrc/align.hip), the inputs the
CPU and GPU tests share, and the checks the GPU test applies.  naturalspeech2_pytorch is absent: parity with it is UNPINNED, the
definitions are the ones include/vbx.h states.

Plain loops over the query frames and, for the path, over the keys of the band.  The loss is differentiable by autograd.  Each
restatement takes `fault=`: a deliberately wrong variant, for tests/test_align_cpu.py to show that the checks would catch it."""
import functools
import math

import torch

NEG = -1e300  # "no probability" in the fp64 loss: finite, so that autograd never sees inf - inf; exp(NEG - anything) is exactly 0
U24 = 2.0 ** -24

PATH_FAULTS = ("tie_moves", "diag_stays", "start_at_K")
LOSS_FAULTS = ("no_skip", "skip_from_blank", "blank_zero", "key_mask_off_by_one", "no_div")


# ----------------------------------------------------------------------------- maximum_path
def path_table(value, q, k, fault=None):
    """Q fp64 [q, k], -inf outside the reachable band max(0, k + y - q) <= x <= min(k - 1, y); a loop over the frames, the keys of
    a frame at once"""
    ninf = -math.inf
    out_of_band = 0.0 if fault == "diag_stays" else ninf  # the fault: a table initialised with zeros, so the diagonal may stay
    v = value.double()
    xs = torch.arange(k)
    Q = torch.full((q, k), ninf, dtype=torch.float64)
    Q[0, 0] = v[0, 0]
    for y in range(1, q):
        prev = Q[y - 1]
        band_prev = (xs >= max(0, k + y - 1 - q)) & (xs <= min(k - 1, y - 1))
        stay = torch.where(band_prev, prev, torch.tensor(out_of_band, dtype=torch.float64))
        move = torch.cat((torch.tensor([ninf], dtype=torch.float64), torch.where(band_prev, prev, torch.tensor(ninf, dtype=torch.float64))[:-1]))
        band = (xs >= max(0, k + y - q)) & (xs <= min(k - 1, y))
        Q[y] = torch.where(band, torch.maximum(stay, move) + v[y, :k], torch.tensor(ninf, dtype=torch.float64))
    return Q


def maximum_path_ref(value, q, k, fault=None):
    """value [T, K] -> (path fp64 [T, K], durations int64 [K], Q); all zeros for a row without a monotonic path"""
    T, K = value.shape
    path = torch.zeros(T, K, dtype=torch.float64)
    if k < 1 or q < k:
        return path, torch.zeros(K, dtype=torch.int64), None
    Q = path_table(value, q, k, fault)
    ninf = -math.inf
    idx = (K if fault == "start_at_K" else k) - 1
    for y in range(q - 1, -1, -1):
        path[y, idx] = 1.0
        if idx != 0 and y > 0:
            a = float(Q[y - 1, idx]) if idx < k else ninf
            b = float(Q[y - 1, idx - 1]) if idx - 1 < k else ninf
            forced = idx == y and fault != "diag_stays"
            if forced or (a <= b if fault == "tie_moves" else a < b):
                idx -= 1
    return path, path.sum(0).to(torch.int64), Q


def maximum_path_batch_ref(value, qlens, klens, fault=None):
    """value [B, T, K] -> (path fp64 [B, T, K], durations int64 [B, K], [optimum score or None], [max |Q| over the band or None])"""
    paths, durs, best, qmax = [], [], [], []
    for b in range(value.shape[0]):
        q, k = int(qlens[b]), int(klens[b])
        p, d, Q = maximum_path_ref(value[b], q, k, fault)
        paths.append(p)
        durs.append(d)
        best.append(None if Q is None else float(Q[q - 1, k - 1]))
        qmax.append(None if Q is None else float(Q[torch.isfinite(Q)].abs().max()))
    return torch.stack(paths), torch.stack(durs), best, qmax


def brute_force_path(value, q, k):
    """every monotonic path of q frames over k keys (key 0 first, key k - 1 last, steps 0 / 1): the best score in fp64 and, among
    the paths that reach it, the one the stay-on-tie backtrack returns -- walking back from the end it stays whenever an optimal
    path stays, i.e. the greatest column sequence read from the last frame to the first"""
    import itertools

    v = value.double()
    best, best_cols = None, None
    for moves in itertools.combinations(range(1, q), k - 1):  # the frames at which the key advances
        cols, c = [], 0
        for y in range(q):
            c += y in moves
            cols.append(c)
        s = sum(float(v[y, cols[y]]) for y in range(q))
        key = (s, tuple(reversed(cols)))
        if best is None or key > best:
            best, best_cols = key, cols
    path = torch.zeros_like(v)
    for y, c in enumerate(best_cols):
        path[y, c] = 1.0
    return path, best[0]


def path_problems(path, durations, qlens, klens):
    """what the GPU test asks of every returned path, as a list of complaints (empty = valid)"""
    bad = []
    B, T, K = path.shape
    if not bool(((path == 0) | (path == 1)).all()):
        bad.append("entries other than 0 / 1")
    if not torch.equal(durations, path.sum(1).to(torch.int64)):
        bad.append("durations != path.sum(1)")
    for b in range(B):
        q, k = int(qlens[b]), int(klens[b])
        p = path[b]
        if k < 1 or q < k:
            if bool(p.any()):
                bad.append(f"row {b}: no monotonic path exists, yet the path is not all zero")
            continue
        if bool(p[q:].any()) or bool(p[:, k:].any()):
            bad.append(f"row {b}: ones outside the lengths")
        if not bool((p[:q].sum(1) == 1).all()):
            bad.append(f"row {b}: not exactly one 1 per live frame")
            continue
        cols = p[:q].argmax(1)
        if int(cols[0]) != 0 or int(cols[-1]) != k - 1:
            bad.append(f"row {b}: runs from key {int(cols[0])} to {int(cols[-1])}, not 0 to {k - 1}")
        step = cols[1:] - cols[:-1]
        if q > 1 and not bool(((step == 0) | (step == 1)).all()):
            bad.append(f"row {b}: a column step outside {{0, 1}}")
    return bad


def path_score(path, value):
    """fp64 score of each row's path: [B]"""
    return (path.double() * value.double()).sum((1, 2))


def path_bound(T, qmax):
    """how far below the fp64 optimum the score of a path that is optimal for the fp32-rounded table may lie: each of the <= T fp32
    additions along either path loses at most half an ulp of a table entry, (2 T + 2) 2^-24 max |Q|"""
    return (2 * T + 2) * U24 * qmax


# ----------------------------------------------------------------------------- forward-sum loss
def _lse3(a, b, c):
    return torch.logsumexp(torch.stack((a, b, c)), 0)


def forward_sum_nll_ref(x, k, q, blank=-1.0, fault=None):
    """x [T, K] (fp64, may require grad) -> -log Z of one row: CTC, blank 0, target 1 .. k, over the log-softmax of
    [blank, x[t][0 .. k)] for the frames t < q; 0 (attached to x) for a row without a monotonic path"""
    T, K = x.shape
    if k < 1 or q < k:
        return x.sum() * 0.0
    if fault == "blank_zero":
        blank = 0.0
    kk = min(k + 1, K) if fault == "key_mask_off_by_one" else k
    z = torch.cat((torch.full((q, 1), blank, dtype=x.dtype), x[:q, :kk]), 1)
    lp = torch.log_softmax(z, 1)
    S = 2 * k + 1
    ext = torch.tensor([0 if s % 2 == 0 else (s + 1) // 2 for s in range(S)])
    lpe = lp[:, ext]  # [q, S]
    if fault == "no_skip":
        skip = torch.zeros(S, dtype=torch.bool)
    elif fault == "skip_from_blank":
        skip = torch.tensor([s >= 2 for s in range(S)])
    else:
        skip = torch.tensor([s % 2 == 1 and s >= 3 for s in range(S)])
    neg = torch.full((S,), NEG, dtype=x.dtype)
    alpha = torch.cat((lpe[0, :2], neg[2:]))
    for t in range(1, q):
        a1 = torch.cat((neg[:1], alpha[:-1]))
        a2 = torch.where(skip, torch.cat((neg[:2], alpha[:-2])), neg)
        alpha = _lse3(alpha, a1, a2) + lpe[t]
    return -torch.logsumexp(alpha[-2:], 0)


def forward_sum_ref(x, klens, qlens, blank=-1.0, reduction="mean", fault=None):
    """x [B, T, K] fp64 -> nll [B] ("none") or mean_b(nll_b / key_len_b) ("mean")"""
    nll = torch.stack([forward_sum_nll_ref(x[b], int(klens[b]), int(qlens[b]), blank, fault) for b in range(x.shape[0])])
    if reduction == "none":
        return nll
    if fault == "no_div":
        return nll.mean()
    return (nll / torch.as_tensor(klens, dtype=x.dtype).clamp(min=1)).mean()


def ctc_construction(x, klens, qlens, blank=-1.0, reduction="mean"):
    """the same loss from torch's own pieces, in x's dtype: pad a blank column, fill the keys past key_len with -finfo.max,
    log_softmax, F.ctc_loss(blank=0, zero_infinity=True) with target 1 .. key_len"""
    import torch.nn.functional as F

    B, T, K = x.shape
    klens, qlens = torch.as_tensor(klens, dtype=torch.int64), torch.as_tensor(qlens, dtype=torch.int64)
    z = F.pad(x, (1, 0), value=blank)
    keep = torch.arange(K + 1)[None, None, :] <= klens[:, None, None]
    z = z.masked_fill(~keep, -torch.finfo(x.dtype).max)
    lp = torch.log_softmax(z, 2).transpose(0, 1)  # [T, B, K + 1]
    targets = torch.arange(1, K + 1)[None, :].expand(B, K)
    return F.ctc_loss(lp, targets, qlens, klens, blank=0, reduction=reduction, zero_infinity=True)


# ----------------------------------------------------------------------------- the inputs both test files use
SHAPES = [(3, 5, 1), (3, 7, 7), (3, 66, 64), (3, 70, 65), (2, 200, 129), (2, 1032, 1024), (2, 2500, 40),
          (3, 63, 9), (3, 64, 9), (3, 65, 9), (3, 129, 9)]  # the last four: the 64-row batches of the backtrack


def length_rows(T, K):
    """(query_len, key_len) of the five kinds of row every shape is run with: full; key_len < K and query_len == key_len + 1 < T;
    query_len == key_len (< T unless T == K); key_len < K with query_len < T and room to spare; infeasible (query_len < key_len).
    At K == 1 `key_len < K` cannot hold for a row that has a path, and key_len stays 1."""
    k1 = max(1, K - 3)
    k2 = max(1, K // 2)
    k3 = max(1, K - 1)
    return [(T, K), (min(T, k1 + 1), k1), (k2, k2), (max(k3, T - 3), k3), (K - 1, K)]


def length_batches(B, T, K):
    """the five rows dealt into batches of B (wrapping): every batch of a shape together covers all five kinds"""
    rows = length_rows(T, K)
    n = -(-len(rows) // B)
    out = []
    for i in range(n):
        pick = [rows[(i * B + j) % len(rows)] for j in range(B)]
        out.append(([p[0] for p in pick], [p[1] for p in pick]))
    return out  # [(qlens, klens)]


def _gen(B, T, K, salt):
    return torch.Generator().manual_seed(1000003 * salt + 7919 * B + 31 * T + K)


def integer_scores(B, T, K):
    """integers in [-3, 3]: every fp32 sum is exact and ties are everywhere"""
    return torch.randint(-3, 4, (B, T, K), generator=_gen(B, T, K, 1)).float()


def gaussian_scores(B, T, K):
    return torch.randn(B, T, K, generator=_gen(B, T, K, 2))


def loss_inputs(B, T, K):
    return 3.0 * torch.randn(B, T, K, generator=_gen(B, T, K, 3))


@functools.lru_cache(maxsize=None)
def path_reference(kind, B, T, K, batch):
    """(value, qlens, klens, path, durations, best, qmax) of one batch of one shape, computed once"""
    value = integer_scores(B, T, K) if kind == "int" else gaussian_scores(B, T, K)
    qlens, klens = length_batches(B, T, K)[batch]
    return (value, qlens, klens) + maximum_path_batch_ref(value, qlens, klens)


@functools.lru_cache(maxsize=None)
def loss_reference(B, T, K, batch, blank=-1.0):
    """one batch of one shape, computed once: the inputs, the fp64 restatement (nll per row, mean, gradient of the mean and of
    sum(nll)) and the error of torch's own fp32 CPU construction against it"""
    x = loss_inputs(B, T, K)
    qlens, klens = length_batches(B, T, K)[batch]
    xd = x.double().requires_grad_(True)
    nll = forward_sum_ref(xd, klens, qlens, blank, "none")
    mean = (nll / torch.tensor(klens, dtype=torch.float64).clamp(min=1)).mean()
    g_sum, = torch.autograd.grad(nll.sum(), xd)
    # the rows are independent, so the gradient of the mean is each row's gradient times 1 / (B key_len): one backward pass
    g_mean = g_sum / (x.shape[0] * torch.tensor(klens, dtype=torch.float64).clamp(min=1))[:, None, None]
    xf = x.clone().requires_grad_(True)
    c_nll = ctc_construction(xf, klens, qlens, blank, "none")
    c_gsum, = torch.autograd.grad(c_nll.sum(), xf)
    xf = x.clone().requires_grad_(True)
    c_mean = ctc_construction(xf, klens, qlens, blank, "mean")
    c_gmean, = torch.autograd.grad(c_mean, xf)
    nll, mean = nll.detach(), mean.detach()
    cpu_err = dict(nll=(c_nll.detach().double() - nll).abs(), mean=float((c_mean.detach().double() - mean).abs()),
                   g_sum=float((c_gsum.double() - g_sum).abs().max()), g_mean=float((c_gmean.double() - g_mean).abs().max()))
    return dict(x=x, qlens=qlens, klens=klens, nll=nll, mean=mean, g_mean=g_mean, g_sum=g_sum, cpu_err=cpu_err)


def loss_tolerances(ref, T):
    """what the GPU test allows: 4 x the error of torch's fp32 CPU construction on the same inputs (x 2 for another summation
    order, doubled because the device's expf / log1pf are not the CPU's), with a floor of T 2^-23 max(1, |nll|) for the loss and
    2^-20 max |grad| for the gradient, so that a lucky CPU arm cannot make the bound vanish"""
    floor_nll = T * 2.0 ** -23 * ref["nll"].abs().clamp(min=1.0)
    floor_mean = T * 2.0 ** -23 * max(1.0, abs(float(ref["mean"])))
    return dict(nll=torch.maximum(4.0 * ref["cpu_err"]["nll"], floor_nll),
                mean=max(4.0 * ref["cpu_err"]["mean"], floor_mean),
                g_sum=max(4.0 * ref["cpu_err"]["g_sum"], 2.0 ** -20 * float(ref["g_sum"].abs().max())),
                g_mean=max(4.0 * ref["cpu_err"]["g_mean"], 2.0 ** -20 * float(ref["g_mean"].abs().max())))
