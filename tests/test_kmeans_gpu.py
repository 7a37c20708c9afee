"""voicebox_pytorch_amd.KMeans / kmeans_plusplus on the device (csrc/kmeans.hip) against the fp64 restatement tests/kmeans_ref.py, which
tests/test_kmeans_cpu.py pins to sklearn.  Every check is teacher-forced on the device's own earlier choices (ids, chosen rows), so a
legitimate near-tie never cascades; every bound is derived where it is used.  Figures are printed as `PARITY ...` lines
(profiles/kmeans_parity.txt holds a recorded run)."""
import functools

import pytest
import torch

import kmeans_ref as KR

gpu = pytest.mark.gpu
dev = "cuda"
U23, U24 = 2.0 ** -23, 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _search(x, c, lens=None, N=None):
    """the device search on x [M, D] (lens: x is [B * N, D]) -> (ids int64 [M] on the CPU, mind fp32 [M] on the CPU)"""
    from voicebox_pytorch_amd import _lib

    M, D = x.shape
    K = c.shape[0]
    xd, cd = x.to(dev).contiguous(), c.to(dev).contiguous()
    norms = torch.empty(K, device=dev)
    ids = torch.full((M,), -7, dtype=torch.int32, device=dev)
    mind = torch.full((M,), -7.0, device=dev)
    st = _lib.current_stream()
    _lib.call("vbx_kmeans_norms", cd, norms, K, D, st)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    _lib.call("vbx_kmeans_search", xd, cd, norms, ld, ids, mind, M, M if N is None else N, D, K, st)
    return ids.cpu().to(torch.int64), mind.cpu()


def _accumulate(x, ids, mind, K):
    """the device accumulate -> (sums [K, D], counts int64 [K], inertia fp64, inertia fp32), on the CPU"""
    from voicebox_pytorch_amd import _lib

    M, D = x.shape
    xd = x.to(dev).contiguous()
    scratch = torch.empty(_lib.lib().vbx_kmeans_accumulate_scratch_bytes(M, D, K), dtype=torch.uint8, device=dev)
    sums, counts = torch.full((K, D), 9.0, device=dev), torch.full((K,), -1, dtype=torch.int32, device=dev)
    i64, i32 = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros((), device=dev)
    _lib.call("vbx_kmeans_accumulate", xd, ids.to(torch.int32).to(dev), mind.to(dev), sums, counts, i64, i32, scratch, M, D, K,
              _lib.current_stream())
    return sums.cpu(), counts.cpu().to(torch.int64), i64.cpu(), i32.cpu()


def _tile(D):
    from voicebox_pytorch_amd import _lib

    return _lib.lib().vbx_kmeans_search_tile(D)


# ------------------------------------------------------------------------------------------------ search
# D: the narrowest; one stage of the codebook stream (32); a stage and a tail of 8; HuBERT base (24 stages); 1024 (stages of 16 beside a
# 32-row tile); 1032 and 2048 (the 16-row tile).  K: 1, 2, 5; one MFMA tile (32 centres of a wave) -+ 1; one stage (128) -+ 1; 500.
@gpu
@pytest.mark.parametrize("D", [8, 32, 40, 768, 1024, 1032, 2048])
def test_search_contract_per_row(D):
    """d(id) - min d <= (D + 2) 2^-23 (|x| + max |c|)^2 per row against fp64 on the same operands (tests/rvq_ref.py derives it), and
    the min distance by differences within (D + 2) 2^-23 of itself: each difference is within 2^-24 relatively, its square within
    2^-23, the sum of D non-negative terms in any order adds (D - 1) 2^-24 -- (D + 2) 2^-24 to first order, doubled for the rest."""
    T = _tile(D)
    worst = worst_d = 0.0
    for K in (1, 2, 5, 31, 33, 127, 129, 500):
        if D >= 1024 and K not in (1, 33, 129, 500):
            continue
        for M in (1, T - 1, T, T + 1):
            g = _gen(1000 * D + 10 * K + M)
            c = torch.randn(K, D, generator=g)
            x = c[torch.randint(0, K, (M,), generator=g)] + 0.7 * torch.randn(M, D, generator=g)
            ids, mind = _search(x, c)
            assert int(ids.min()) >= 0 and int(ids.max()) < K, (K, M)
            res = KR.check_search(x, c, ids)
            assert res["violations"] == 0 and res["forced_wrong"] == 0, (K, M, res)
            d64 = KR.distances(x, c)[torch.arange(M), ids]
            rel = ((mind.double() - d64).abs() / d64.clamp(min=1e-300)).max()
            assert float(rel) <= (D + 2) * U23, (K, M, float(rel))
            worst, worst_d = max(worst, res["worst"]), max(worst_d, float(rel) / ((D + 2) * U23))
    print(f"PARITY search D {D}: worst regret / bound {worst:.3e}, worst min-distance error / bound {worst_d:.3e}")


@gpu
def test_search_exact_ties_take_the_lowest_index():
    """duplicated centres in another lane, another wave's 32 and another stage of 128: identical computed distances, the first wins"""
    g = _gen(5)
    K, D = 300, 40
    c = torch.randn(K, D, generator=g)
    pairs = ((3, 7), (10, 50), (0, 290), (129, 255), (64, 63 + 128))
    for lo, hi in pairs:
        c[hi] = c[lo]
    near = torch.tensor([p[i] for p in pairs for i in (0, 1) for _ in range(9)] + [17] * 9)
    x = c[near] + 0.05 * torch.randn(near.numel(), D, generator=g)
    ids, _ = _search(x, c)
    want = torch.tensor([p[0] for p in pairs for _ in range(18)] + [17] * 9)
    assert torch.equal(ids, want)


@gpu
def test_search_near_ties_inside_the_bound_accept_either():
    """pairs of centres one fp32 ulp apart in one component: the fp64 gap is far inside the bound, either id meets the contract"""
    g = _gen(6)
    K, D, M = 64, 72, 99
    base = torch.randn(K // 2, D, generator=g)
    other = base.clone()
    other[:, 5] = torch.nextafter(other[:, 5], torch.full_like(other[:, 5], 10.0))
    c = torch.stack((base, other), dim=1).reshape(K, D)
    x = base[torch.randint(0, K // 2, (M,), generator=g)] + 0.3 * torch.randn(M, D, generator=g)
    ids, _ = _search(x, c)
    res = KR.check_search(x, c, ids)
    assert res["violations"] == 0 and res["forced"] == 0, res
    d = KR.distances(x, c)
    assert bool((ids // 2 == d.argmin(1) // 2).all())  # the right pair, either member


@gpu
@pytest.mark.parametrize("Mp,Dp,Kp,seed", KR.PLANTED)
def test_search_planted_gaps_force_the_fp64_argmin(Mp, Dp, Kp, seed):
    """gaps of 1.5 .. 6 bounds, on which ONE fp16 rounding of the operands fails (tests/test_kmeans_cpu.py): the id IS the fp64 argmin"""
    x, c = KR.planted(Mp, Dp, Kp, seed)
    ids, _ = _search(x, c)
    res = KR.check_search(x, c, ids)
    print(f"PARITY planted D {Dp} K {Kp}: {res}")
    assert res["violations"] == 0 and res["forced_wrong"] == 0 and res["forced"] == Mp, res
    assert torch.equal(ids, KR.assign(x, c)[0])


@gpu
def test_search_dead_rows_are_never_read():
    g = _gen(7)
    B, N, D, K = 4, 37, 40, 9
    lens = [37, 0, 5, 33]
    c = torch.randn(K, D, generator=g)
    x = torch.randn(B, N, D, generator=g)
    live = KR.live_rows(lens, N)
    noisy = x.reshape(-1, D).clone()
    noisy[~live] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e38] * (D // 4))
    ids, mind = _search(noisy, c, lens=lens, N=N)
    ids0, mind0 = _search(x.reshape(-1, D), c)
    assert bool((ids[~live] == K).all()) and bool((mind[~live] == 0).all())
    assert torch.equal(ids[live], ids0[live]) and torch.equal(mind[live], mind0[live])


# ------------------------------------------------------------------------------------------------ accumulate
@functools.lru_cache(maxsize=None)
def _acc_case():
    """M = 777 rows (four sort tiles of 256, twenty-five search tiles), D = 72; centre 0 far from everything (empty), centre 1 ON an
    outlier row (one member), centre 2 in the bulk: all the others -- 776 members, thirteen partial sums; plus three centres far away"""
    g = _gen(8)
    M, D = 777, 72
    x = torch.randn(M, D, generator=g)
    x[17] += 40.0
    c = torch.stack([torch.full((D,), -90.0), x[17].clone(), x[torch.arange(M) != 17].mean(0), torch.full((D,), 70.0),
                     torch.full((D,), -70.0), torch.full((D,), 55.0)])
    return x, c


def _check_sums(x, ids, sums, counts, K, tag):
    S, A, n = KR.sums_counts(x, ids, K)
    assert torch.equal(counts, n), tag
    bound = n.double()[:, None] * U24 * A
    err = (sums.double() - S).abs()
    assert bool((err <= bound).all()), (tag, float((err - bound).max()))
    assert bool((sums[n == 0] == 0).all()), tag
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"PARITY accumulate {tag}: worst |S - S64| / (n 2^-24 sum|x|) {ratio:.3e}, counts {sorted(set(n.tolist()))[:6]}")


@gpu
def test_accumulate_per_element_against_fp64():
    """teacher-forced on the device's own ids: |S - S64| <= n 2^-24 sum |x| per element (n - 1 additions in any order, each within
    2^-24 of a partial sum no larger than sum |x|); counts exact; clusters with 0, 1 and (almost) all members; K = 1: all M"""
    x, c = _acc_case()
    ids, mind = _search(x, c)
    K = c.shape[0]
    assert torch.bincount(ids, minlength=K).tolist() == [0, 1, 776, 0, 0, 0]
    sums, counts, i64, i32 = _accumulate(x, ids, mind, K)
    _check_sums(x, ids, sums, counts, K, "0 / 1 / 776 members")
    assert float(i32) == float(i64.float()) and abs(float(i64) - float(mind.double().sum())) <= 1e-12 * float(mind.double().sum())
    again = _accumulate(x, ids, mind, K)
    assert all(torch.equal(a, b) for a, b in zip((sums, counts, i64, i32), again))  # the same bits on a rerun
    ids1, mind1 = _search(x, c[2:3])
    sums1, counts1, _, _ = _accumulate(x, ids1, mind1, 1)
    assert counts1.tolist() == [777]
    _check_sums(x, ids1, sums1, counts1, 1, "all 777 rows in one cluster")
    g = _gen(9)
    cr = torch.randn(37, 72, generator=g)
    idr, mindr = _search(x, cr)
    sr, cr_n, _, _ = _accumulate(x, idr, mindr, 37)
    _check_sums(x, idr, sr, cr_n, 37, "37 random centres")
    idr[::5] = 37  # dead rows, as the search marks them
    sr, cr_n, _, _ = _accumulate(x, idr, mindr, 37)
    _check_sums(x, idr, sr, cr_n, 37, "37 random centres, every fifth row dead")


def _km(c, w=None):
    import voicebox_pytorch_amd as vbx

    km = vbx.KMeans(c.shape[0], c.shape[1], init=c)
    if w is not None:
        km.load_state_dict(dict(cluster_centers=c, counts=w))
    return km


@gpu
def test_batch_shape_does_not_move_a_bit():
    """the same rows as [M, D], as [B, N, D] and as [B, N, D] with full lens: centres, counts and inertia bit-equal"""
    x, c = _acc_case()
    x = x[:330]
    outs = []
    for feats, lens in ((x, None), (x.reshape(10, 33, 72), None), (x.reshape(3, 110, 72), [110, 110, 110]),
                        (x.reshape(33, 10, 72), torch.full((33,), 10, device=dev))):
        km = _km(c).partial_fit(feats.to(dev), lens=lens)
        outs.append((km.cluster_centers_.cpu(), km.counts_.cpu(), km.inertia_.cpu(), km.labels_.cpu()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))


# ------------------------------------------------------------------------------------------------ update
@gpu
def test_update_bounds_and_empty_centres():
    """Minibatch c' = (c (float)w + S) / (float)(w + n) against fp64 from the exact sums, teacher-forced on the device's ids:
    |c' - c'64| <= (n + 6) 2^-24 (|c| w + sum |x|) / (w + n).  Derivation, u = 2^-24, relative to the numerator N = |c| w + sum |x|:
    S is within n u sum |x| (accumulate's bound); (float)w and (float)(w + n) are within u each; the product c * wf, the addition and
    the correctly rounded division round once each: 2 conversions + 3 operations = 5 u N, and one more for the second-order terms:
    (n + 6) u N / (w + n).  Lloyd c' = S / (float)n: n u from S, the conversion of n (exact below 2^24) and the division: (n + 2) u
    sum |x| / n.  A centre without members keeps its bits."""
    x, c = _acc_case()
    K = c.shape[0]
    w = torch.tensor([5, 0, 3, (1 << 33) + 1, 77, 1000])
    km = _km(c, w).partial_fit(x.to(dev))
    ids = km.labels_.cpu().to(torch.int64)
    S, A, n = KR.sums_counts(x, ids, K)
    assert n.tolist() == [0, 1, 776, 0, 0, 0]
    c64, w64 = c.double(), w.double()
    want = (c64 * w64[:, None] + S) / (w64 + n)[:, None].clamp(min=1)
    bound = (n + 6).double()[:, None] * U24 * (c64.abs() * w64[:, None] + A) / (w64 + n)[:, None].clamp(min=1)
    got = km.cluster_centers_.cpu()
    live = n > 0
    err = (got.double() - want).abs()
    assert bool((err[live] <= bound[live]).all()), float((err[live] / bound[live]).max())
    assert torch.equal(got[~live], c[~live])  # bit-unchanged
    assert torch.equal(km.counts_.cpu(), w + n) and km.n_steps_ == 1
    print(f"PARITY minibatch update: worst error / bound {float((err[live] / bound[live].clamp(min=1e-300)).max()):.3e}")
    kl = _km(c, w).fit(x.to(dev), n_iter=1)
    assert torch.equal(kl.labels_.cpu().to(torch.int64), ids)
    got = kl.cluster_centers_.cpu()
    want = S / n.double()[:, None].clamp(min=1)
    bound = (n + 2).double()[:, None] * U24 * A / n.double()[:, None].clamp(min=1)
    err = (got.double() - want).abs()
    assert bool((err[live] <= bound[live]).all()), float((err[live] / bound[live]).max())
    assert torch.equal(got[~live], c[~live]) and torch.equal(kl.counts_.cpu(), n)
    print(f"PARITY lloyd update: worst error / bound {float((err[live] / bound[live].clamp(min=1e-300)).max()):.3e}")


# ------------------------------------------------------------------------------------------------ lens
@gpu
@pytest.mark.parametrize("device_lens", [False, True])
def test_lens_is_the_live_rows_alone(device_lens):
    """the padding holds noise, inf and NaN; centres, counts and inertia are bit-equal to the call on the live rows concatenated"""
    g = _gen(10)
    B, N, D, K = 6, 50, 40, 7
    lens = [50, 0, 13, 49, 1, 50]
    x = torch.randn(B, N, D, generator=g) + 3.0 * torch.randn(B, N, 1, generator=g)
    c = x.reshape(-1, D)[torch.tensor([0, 3, 110, 160, 200, 251, 299])].clone()  # live rows
    live = KR.live_rows(lens, N)
    alone = x.reshape(-1, D)[live]
    noisy = x.clone().reshape(-1, D)
    junk = torch.randn(int((~live).sum()), D, generator=g) * 1e3
    junk[::3] = float("nan")
    junk[1::3, ::2] = float("inf")
    noisy[~live] = junk
    noisy = noisy.reshape(B, N, D).to(dev)
    ld = torch.tensor(lens, device=dev) if device_lens else lens
    for lloyd in (False, True):
        a, b = _km(c), _km(c)
        if lloyd:
            a.fit(noisy, n_iter=2, lens=ld), b.fit(alone.to(dev), n_iter=2)
        else:
            for _ in range(2):
                a.partial_fit(noisy, lens=ld), b.partial_fit(alone.to(dev))
        assert torch.isfinite(a.cluster_centers_).all()
        assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.counts_, b.counts_)
        assert torch.equal(a.inertia_, b.inertia_) and float(a.inertia_) > 0
        assert torch.equal(a.labels_.cpu()[live], b.labels_.cpu()) and bool((a.labels_.cpu()[~live] == K).all())
        assert int(a.counts_.sum()) == sum(lens) * (1 if lloyd else 2)
    if device_lens:  # out-of-range device lens are clamped into 0 .. N
        a = _km(c).partial_fit(noisy, lens=torch.tensor([77, -4, 13, 49, 1, 50], device=dev))
        b = _km(c).partial_fit(alone.to(dev))
        assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.counts_, b.counts_)


# ------------------------------------------------------------------------------------------------ three steps
@gpu
def test_three_partial_fit_steps_from_a_given_init():
    """Blobs of spread 0.5 around centres of std 4 in D = 40: every row's fp64 margin to its second-nearest centre exceeds the search
    bound at every step (asserted first), so the ids must EQUAL the restatement's; counts exact; the centres inside the accumulated
    bound e_t = e_{t-1} w / (w + n) + (n + 6) 2^-24 (|c| w + sum |x|) / (w + n) (the update's own bound plus what the previous
    step's error contributes through c w / (w + n))."""
    Mb, D, K = 400, 40, 12
    x, centres, _ = KR.blobs(3 * Mb, D, K, spread=0.5, seed=21)
    init = (centres + 0.3 * torch.randn(K, D, generator=_gen(22))).float()
    km = _km(init)
    c64, w64 = init.double(), torch.zeros(K, dtype=torch.int64)
    err_bound = torch.zeros(K, D, dtype=torch.float64)
    for t in range(3):
        xb = x[t * Mb:(t + 1) * Mb]
        dev_c = km.cluster_centers_.cpu() if t else init
        for cc in (c64, dev_c):  # the margin holds for the restatement's centres and for the device's own
            assert bool((KR.margins(xb, cc) > 4 * KR.search_bound(xb, cc)).all()), t
        _, A, n = KR.sums_counts(xb, KR.assign(xb, c64)[0], K)
        den = (w64 + n).double().clamp(min=1)[:, None]
        step = (n + 6).double()[:, None] * U24 * (c64.abs() * w64.double()[:, None] + A) / den
        err_bound = torch.where((n > 0)[:, None], err_bound * w64.double()[:, None] / den + step, err_bound)
        c64, w64, ids64, _ = KR.minibatch_step(xb, c64, w64)
        inertia64 = float(KR.assign(xb, dev_c)[1].sum())  # with the centres the device measured it with
        km.partial_fit(xb.to(dev))
        assert torch.equal(km.labels_.cpu().to(torch.int64), ids64), t
        assert torch.equal(km.counts_.cpu(), w64), t
        err = (km.cluster_centers_.cpu().double() - c64).abs()
        assert bool((err <= err_bound).all()), (t, float((err / err_bound.clamp(min=1e-300)).max()))
        assert abs(float(km.inertia_) - inertia64) <= (D + 4) * U23 * inertia64, t
        print(f"PARITY partial_fit step {t}: worst centre error / bound {float((err / err_bound.clamp(min=1e-300)).max()):.3e}, "
              f"inertia {float(km.inertia_):.6e} vs fp64 {inertia64:.6e}")
    assert km.n_steps_ == 3 and int(w64.min()) > 0


# ------------------------------------------------------------------------------------------------ k-means++
def _check_plusplus(x2, K, u, idx, live=None):
    """teacher-forced on the earlier indices: with P64 the fp64 running sum of p over ascending rows, the picked row i of step j has
    P64[i] >= u_j sum(P) - s and P64[i - 1] <= u_j sum(P) + s,  s = sum_i (D + 2) 2^-23 (|x_i| + max |x|)^2 + M 2^-23 sum(P): the first
    term is every p_i's own fp32 error (the search contract's form: differences, squares, a sum of D terms), the second a running
    sum of M terms in any order and precision down to fp32 plus the product u_j * total.  No row repeats while sum(p) > 0; dead rows
    are never picked."""
    M, D = x2.shape
    idx = [int(i) for i in idx]
    rows = torch.arange(M) if live is None else torch.nonzero(live).reshape(-1)
    assert idx[0] == int(rows[min(int(float(u[0]) * len(rows)), len(rows) - 1)])
    nrm = x2.double().norm(dim=1)
    s_rows = float(((D + 2) * U23 * (nrm + nrm.max()) ** 2)[rows].sum())
    worst = 0.0
    for j in range(1, K):
        i = idx[j]
        assert live is None or bool(live[i]), (j, i)
        p = KR.pp_potential(x2, idx[:j], live)
        cum = torch.cumsum(p, 0)
        total = float(cum[-1])
        if total > 0:
            assert i not in idx[:j] and float(p[i]) > 0, (j, i)
            s, target = s_rows + M * U23 * total, float(u[j]) * total
            assert float(cum[i]) >= target - s and (float(cum[i - 1]) if i else 0.0) <= target + s, (j, i)
            exact = int(torch.nonzero((cum >= target) & (p > 0))[0])
            worst = max(worst, abs(float(cum[i]) - float(cum[exact])) / s)
        else:
            assert i == int(rows[min(int(float(u[j]) * len(rows)), len(rows) - 1)]), (j, i)
    return worst


@gpu
def test_plusplus_with_given_u():
    from voicebox_pytorch_amd import kmeans_plusplus

    g = _gen(30)
    B, N, D, K = 5, 70, 24, 20
    lens = [70, 0, 33, 69, 1]
    x = torch.randn(B, N, D, generator=g) * 2.0
    live = KR.live_rows(lens, N)
    x.reshape(-1, D)[~live] = float("nan")
    u = torch.rand(K, generator=g)
    u[3], u[4] = 0.0, 1.0 - 2.0 ** -24  # both ends of the running sum
    for lens_arg in (lens, torch.tensor(lens, device=dev)):
        centers, idx = kmeans_plusplus(x.to(dev), K, u=u.to(dev), lens=lens_arg)
        assert idx.dtype == torch.int64 and idx.device.type == "cuda"
        idx = idx.cpu()
        assert torch.equal(centers.cpu(), x.reshape(-1, D)[idx])
        worst = _check_plusplus(torch.nan_to_num(x.reshape(-1, D), nan=0.0), K, u, idx, live)
    print(f"PARITY kmeans_plusplus ragged: worst |P64[i] - P64[i*]| / s {worst:.3e}")
    x2 = torch.randn(1000, 16, generator=g)
    centers2, idx2 = kmeans_plusplus(x2.to(dev), 30, seed=5)  # u drawn on the device from the seed: the same draw, the same picks
    centers3, idx3 = kmeans_plusplus(x2.to(dev), 30, seed=5)
    assert torch.equal(idx2, idx3) and torch.equal(centers2, centers3) and len(set(idx2.tolist())) == 30


@gpu
def test_plusplus_blocks_of_the_running_sum():
    from voicebox_pytorch_amd import kmeans_plusplus

    g = _gen(31)
    x = torch.randn(1000, 16, generator=g)  # sixteen blocks of 64 rows
    u = torch.rand(30, generator=g)
    _, idx = kmeans_plusplus(x.to(dev), 30, u=u)
    worst = _check_plusplus(x, 30, u, idx.cpu())
    print(f"PARITY kmeans_plusplus 1000 rows: worst |P64[i] - P64[i*]| / s {worst:.3e}")


@gpu
def test_plusplus_one_row_per_blob_and_the_degenerate_cases():
    """8 blobs of 8 rows, centres of std 10 and noise of std 1e-5 in D = 8.  A miss at step j has probability (sum of p over the rows
    of the blobs already hit) / sum(p) <= 56 * max within-blob d^2 / (8 * min between-blob d^2): within-blob d^2 is about 2 D sigma^2
    = 1.6e-9, between-blob d^2 about 2 D 100 = 1600, so about 7e-12 per step; the test computes the exact sum over the seven steps
    in fp64 on these very rows and requires it below 1e-9 before it looks at which blobs the device hit."""
    from voicebox_pytorch_amd import kmeans_plusplus

    x, _, which = KR.blobs(64, 8, 8, spread=1e-5, seed=3, scale=10.0)
    u = torch.rand(8, generator=_gen(4))
    _, idx = kmeans_plusplus(x.to(dev), 8, u=u)
    idx = idx.cpu().tolist()
    miss = 0.0
    for j in range(1, 8):
        p = KR.pp_potential(x, idx[:j])
        hit = torch.isin(which, which[torch.tensor(idx[:j])])
        miss += float(p[hit].sum() / p.sum())
    assert miss < 1e-9, miss
    assert sorted(int(which[i]) for i in idx) == list(range(8))
    _check_plusplus(x, 8, u, idx)
    # M_live == K: every live row exactly once
    xl = torch.randn(3, 6, 8, generator=_gen(5))
    lens = [2, 0, 6]
    _, idx = kmeans_plusplus(xl.to(dev), 8, u=torch.rand(8, generator=_gen(6)), lens=lens)
    assert sorted(idx.cpu().tolist()) == [0, 1, 12, 13, 14, 15, 16, 17]
    # all rows equal: sum(p) == 0 from step 1 on -> floor(u_j M)
    same = torch.ones(12, 8)
    _, idx = kmeans_plusplus(same.to(dev), 3, u=torch.tensor([0.0, 0.5, 0.99]))
    assert idx.cpu().tolist() == [0, 6, 11]


# ------------------------------------------------------------------------------------------------ the public paths
@gpu
def test_init_variants_predict_and_no_host_synchronisation():
    import voicebox_pytorch_amd as vbx

    x, _, which = KR.blobs(640, 24, 8, spread=0.005, seed=40, scale=6.0)
    xd = x.reshape(8, 80, 24).to(dev)
    lens = torch.tensor([80, 0, 13, 80, 79, 1, 80, 80], device=dev)
    live = KR.live_rows(lens.cpu(), 80)
    u = torch.rand(8, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        kp = vbx.KMeans(8, 24, init="k-means++", seed=1).partial_fit(xd, lens=lens)
        kr = vbx.KMeans(8, 24, init="random", seed=1).partial_fit(xd, lens=lens).fit(xd, n_iter=3, lens=lens)
        ids = kp.predict(xd)
        vbx.kmeans_plusplus(xd, 8, u=u, lens=lens)
        vbx.kmeans_plusplus(xd, 8, seed=3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # k-means++ on separated blobs finds one row per blob; a step later every centre is its blob's mean over the live rows
    assert int(kp.counts_.sum()) == int(live.sum()) and int(kp.counts_.min()) > 0
    ids = ids.cpu().reshape(-1)
    assert all(len(set(ids[live & (which == b)].tolist())) == 1 for b in range(8)) and len(set(ids[live].tolist())) == 8
    assert torch.equal(kp.labels_.cpu().to(torch.int64)[live], ids[live])
    # "random": eight distinct live rows, whatever they are; three Lloyd steps leave counts of the last iteration
    assert int(kr.counts_.sum()) == int(live.sum()) and kr.n_steps_ == 4 and torch.isfinite(kr.cluster_centers_).all()
    a = vbx.KMeans(8, 24, init="random", seed=7).partial_fit(xd, lens=lens)
    b = vbx.KMeans(8, 24, init="random", seed=7).partial_fit(xd, lens=lens)
    assert torch.equal(a.cluster_centers_, b.cluster_centers_)


@gpu
def test_hubert_fit_kmeans_on_two_ragged_batches():
    import hubert_ref as R
    import voicebox_pytorch_amd as vbx

    tok = vbx.HubertWithKmeans(**R.SMALL, output_layer=4, codebook_size=64)
    tok.load_state_dict(R.small_state_dict())
    tok = tok.to(dev)
    before = tok.cluster_centers.clone()
    batches = [(R.make_wave(3, 9000, 1).to(dev), [9000, 4000, 7777]), (R.make_wave(2, 6000, 2).to(dev), torch.tensor([6000, 2500]))]
    km = tok.fit_kmeans(batches, n_clusters=16, seed=3)
    frames = sum(sum(tok.frame_lens(list(int(v) for v in l))) for _, l in batches)
    assert tok.codebook_size == 16 and tuple(tok.cluster_centers.shape) == (16, 128) and tok.cluster_centers.shape != before.shape
    assert torch.equal(tok.cluster_centers, km.cluster_centers_) and torch.isfinite(tok.cluster_centers).all()
    assert int(km.counts_.sum()) == frames and km.n_steps_ == 2
    wave, lens = batches[0]
    ids = tok(wave, lens=lens)
    assert ids.dtype == torch.int64 and int(ids.min()) >= 0 and int(ids.max()) < 16
    fl = tok.frame_lens(lens)
    h = tok.features(wave, lens=lens)
    for b, f in enumerate(fl):
        assert torch.equal(ids[b, :f], km.predict(h[b, :f]))
