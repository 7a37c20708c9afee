"""k-means fitting restated in fp64 -- the yardstick of voicebox_pytorch_amd.KMeans / kmeans_plusplus (csrc/kmeans.hip).

PINNED: tests/test_kmeans_cpu.py holds minibatch_step to sklearn's MiniBatchKMeans.partial_fit (reassignment_ratio = 0, init = array)
and lloyd_step to sklearn's KMeans(algorithm="lloyd", init=array, n_init=1, tol=0) within 1e-12 on inputs without an empty cluster.
UNPINNED: plusplus -- the plain D^2 sampling of Arthur & Vassilvitskii with given uniforms, not sklearn's greedy variant.

    assign       with the OLD centres, Euclidean, the lowest index on a tie
    minibatch    c <- (c w + sum of members) / (w + n), w <- w + n;  a centre without members stays where it is
    lloyd        c <- sum of members / n;                             a centre without members stays where it is
Dead rows (live == False) take no part in anything.  The search contract and its checker are vbx_rvq_encode's (tests/rvq_ref.py)."""
import numpy as np
import torch

import rvq_ref as rr

U23, U24 = 2.0 ** -23, 2.0 ** -24
FAULTS = ("assign_updated", "forget_w", "counts_not_carried", "dead_counted", "empty_zeroed", "mean_over_N")


def distances(x, c):
    """|x_m - c_k|^2 in fp64 by differences: x [M, D], c [K, D] -> [M, K]"""
    x, c = x.double(), c.double()
    return torch.stack([((x - c[k]) ** 2).sum(1) for k in range(c.shape[0])], dim=1)


def assign(x, c):
    """-> (ids int64 [M]: the first of equal minima, min distance fp64 [M])"""
    d = distances(x, c)
    ids = torch.from_numpy(np.argmin(d.numpy(), axis=1))
    return ids, d[torch.arange(d.shape[0]), ids]


def search_bound(x, c):
    """the slack of the search contract per row: (D + 2) * 2^-23 * (|x| + max |c|)^2"""
    return (x.shape[-1] + 2) * U23 * (x.double().norm(dim=-1) + c.double().norm(dim=-1).max()) ** 2


def margins(x, c):
    """per row the fp64 gap between the nearest and the second nearest centre (inf for K = 1)"""
    d = distances(x, c)
    if d.shape[1] < 2:
        return torch.full((d.shape[0],), float("inf"), dtype=torch.float64)
    two = torch.topk(d, 2, dim=1, largest=False).values
    return two[:, 1] - two[:, 0]


def check_search(x, c, ids):
    """rvq_ref.check_search for one stage: dict(violations, worst, forced, forced_wrong)"""
    if c.shape[0] == 1:  # nothing to choose from
        wrong = int((ids != 0).sum())
        return dict(violations=wrong, worst=0.0, forced=x.shape[0], forced_wrong=wrong)
    return rr.check_search(x, c[None], ids.to(torch.int64).reshape(-1, 1))


def sums_counts(x, ids, K):
    """per-cluster fp64 sums [K, D], sums of |x| [K, D] and counts int64 [K] of the rows with 0 <= id < K"""
    x = x.double()
    ok = (ids >= 0) & (ids < K)
    S, A = torch.zeros(K, x.shape[1], dtype=torch.float64), torch.zeros(K, x.shape[1], dtype=torch.float64)
    S.index_add_(0, ids[ok], x[ok])
    A.index_add_(0, ids[ok], x[ok].abs())
    return S, A, torch.bincount(ids[ok], minlength=K)


def minibatch_step(x, c, w, live=None, fault=None):
    """one MiniBatchKMeans.partial_fit step at reassignment_ratio = 0: x [M, D], c fp64 [K, D], w int64 [K], live bool [M] or None
    -> (c', w', ids [M] with K for a dead row, inertia).  fault: one of FAULTS, a step that gets exactly that wrong."""
    c, K, M = c.double(), c.shape[0], x.shape[0]
    live = torch.ones(M, dtype=torch.bool) if live is None or fault == "dead_counted" else live
    ids, dmin = assign(x, c)
    ids = torch.where(live, ids, torch.full_like(ids, K))
    S, _, n = sums_counts(x, ids, K)
    if fault == "assign_updated":  # a second pass with the centres the first one produced
        c1 = minibatch_step(x, c, w, live)[0]
        ids = torch.where(live, assign(x, c1)[0], torch.full_like(ids, K))
        S, _, n = sums_counts(x, ids, K)
    w_old = torch.zeros_like(w) if fault == "forget_w" else w
    den = (w_old + n).double()
    if fault == "mean_over_N":
        den = (w_old + int(live.sum())).double().expand(K).clone()
    new = (c * w_old.double()[:, None] + S) / den.clamp(min=1)[:, None]
    keep = n == 0
    c_new = torch.where(keep[:, None], torch.zeros_like(c) if fault == "empty_zeroed" else c, new)
    w_new = n.clone() if fault == "counts_not_carried" else w + n
    return c_new, w_new, ids, float(dmin[live].sum())


def lloyd_step(x, c, live=None, fault=None):
    """one full-batch step c <- mean of the members -> (c', n, ids, inertia)"""
    c, K, M = c.double(), c.shape[0], x.shape[0]
    live = torch.ones(M, dtype=torch.bool) if live is None or fault == "dead_counted" else live
    ids, dmin = assign(x, c)
    ids = torch.where(live, ids, torch.full_like(ids, K))
    S, _, n = sums_counts(x, ids, K)
    den = n.double() if fault != "mean_over_N" else torch.full((K,), float(live.sum()), dtype=torch.float64)
    keep = n == 0
    c_new = torch.where(keep[:, None], torch.zeros_like(c) if fault == "empty_zeroed" else c, S / den.clamp(min=1)[:, None])
    return c_new, n, ids, float(dmin[live].sum())


def live_rows(lens, N):
    """bool [B * N]: row b * N + n lives iff n < lens[b]"""
    return (torch.arange(N)[None, :] < torch.as_tensor(lens)[:, None]).reshape(-1)


def pp_potential(x, chosen, live=None):
    """p_i = min over the chosen rows of |x_i - x_c|^2 in fp64, 0 for a dead row"""
    x = x.double()
    p = distances(x, x[torch.as_tensor(chosen, dtype=torch.int64)]).min(dim=1).values
    return p if live is None else torch.where(live, p, torch.zeros_like(p))


def plusplus(x, K, u, live=None):
    """D^2 sampling with given uniforms u [K] in fp64: step 0 picks live row floor(u_0 M_live); step j the first row with p > 0 whose
    running sum (np.cumsum, ascending rows) reaches u_j sum(p); sum(p) == 0: live row floor(u_j M_live).  -> indices (list)"""
    M = x.shape[0]
    rows = torch.arange(M) if live is None else torch.nonzero(live).reshape(-1)
    u = [float(v) for v in u]
    chosen = [int(rows[min(int(u[0] * len(rows)), len(rows) - 1)])]
    for j in range(1, K):
        p = pp_potential(x, chosen, live).numpy()
        cum = np.cumsum(p)
        if cum[-1] > 0:
            ok = np.nonzero((cum >= u[j] * cum[-1]) & (p > 0))[0]
            chosen.append(int(ok[0]))
        else:
            chosen.append(int(rows[min(int(u[j] * len(rows)), len(rows) - 1)]))
    return chosen


def blobs(M, D, K, spread, seed, scale=4.0):
    """M rows around K centres drawn with std `scale`, isotropic noise of std `spread`; every centre gets rows (round robin, then
    shuffled) -> (x fp32 [M, D], centres fp32 [K, D], the blob of every row)"""
    g = torch.Generator().manual_seed(seed)
    centres = scale * torch.randn(K, D, generator=g)
    which = torch.arange(M) % K
    which = which[torch.randperm(M, generator=g)]
    return (centres[which] + spread * torch.randn(M, D, generator=g)).float(), centres.float(), which


# (M, D, K, seed): the contract's bound grows with D^2 (D 2^-23 |x|^2) while one fp16 rounding of the operands errs like D 2^-11: only at
# modest D does the bound sit below that fault, so the teeth are cut there (tests/rvq_ref.py PLANTED, the same two shapes)
PLANTED = [(256, 32, 64, 200), (256, 128, 1024, 201)]


def planted(M, D, K, seed):
    """rvq_ref.planted: near-ties of 1.5 .. 6 bounds on which ONE fp16 rounding of the operands fails the contract -> (x, c)"""
    x, cb = rr.planted(M, D, K, seed)
    return x, cb[0]


def search_emulated(x, c, mode):
    """rvq_ref.search for one stage: "fp32" (the class the kernel is in) or "fp16" (one rounding of both operands) -> ids"""
    return rr.search(x, c[None], mode)[0][:, 0]
