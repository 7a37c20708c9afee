"""k-means fitting without a GPU: the fp64 restatement tests/kmeans_ref.py against sklearn itself (this PINS the yardstick of
tests/test_kmeans_gpu.py), the faults the restatement must feel, the search contract's teeth, and the host logic of KMeans /
kmeans_plusplus / HubertWithKmeans.fit_kmeans (limits, lens validation, init variants, save -> load_kmeans), all of which arrive
before a device is needed."""
import os

import pytest
import torch

import kmeans_ref as KR

import voicebox_pytorch_amd as vbx
from voicebox_pytorch_amd import KMeans, kmeans_plusplus
from voicebox_pytorch_amd._lib import VbxError
from voicebox_pytorch_amd.hubert import load_kmeans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, D, K = 300, 24, 16


def _case():
    """three batches of 300 rows around 16 blobs and an init near the blobs' centres: no cluster is ever empty (asserted by the users)"""
    x, centres, _ = KR.blobs(3 * M, D, K, spread=1.5, seed=11)
    g = torch.Generator().manual_seed(12)
    init = (centres + 0.5 * torch.randn(K, D, generator=g)).double()
    return x.double(), init


def _run_minibatch(x, init, fault=None, live=None):
    c, w, hist = init.clone(), torch.zeros(K, dtype=torch.int64), []
    for b in range(3):
        c, w, ids, _ = KR.minibatch_step(x[b * M:(b + 1) * M], c, w, live=live, fault=fault)
        hist.append(torch.bincount(ids[ids < K], minlength=K))
    return c, w, hist


# ------------------------------------------------------------------------------------------------ the restatement against sklearn
def test_minibatch_restatement_is_sklearn_partial_fit():
    cluster = pytest.importorskip("sklearn.cluster")
    x, init = _case()
    c, w, hist = _run_minibatch(x, init)
    assert all(int(h.min()) > 0 for h in hist), "an empty cluster: sklearn and the restatement may differ by design"
    mb = cluster.MiniBatchKMeans(n_clusters=K, init=init.numpy(), n_init=1, reassignment_ratio=0.0, batch_size=M, random_state=0)
    for b in range(3):
        mb.partial_fit(x[b * M:(b + 1) * M].numpy())
    err = float((torch.from_numpy(mb.cluster_centers_) - c).abs().max())
    print(f"PARITY MiniBatchKMeans.partial_fit x 3 vs restatement: max |delta| {err:.3e}")
    assert err <= 1e-12, err
    assert torch.equal(torch.from_numpy(mb._counts).to(torch.int64), w)


@pytest.mark.parametrize("iters", [1, 5])
def test_lloyd_restatement_is_sklearn_kmeans(iters):
    cluster = pytest.importorskip("sklearn.cluster")
    x, init = _case()
    x = x[:M]
    c = init.clone()
    for _ in range(iters):
        c, n, _, _ = KR.lloyd_step(x, c)
        assert int(n.min()) > 0, "an empty cluster: sklearn relocates it, the restatement does not"
    km = cluster.KMeans(n_clusters=K, init=init.numpy(), n_init=1, tol=0, max_iter=iters, algorithm="lloyd").fit(x.numpy())
    err = float((torch.from_numpy(km.cluster_centers_) - c).abs().max())
    print(f"PARITY KMeans(lloyd) {iters} iterations vs restatement: max |delta| {err:.3e}")
    assert err <= 1e-12, err


def test_planted_faults_move_the_centres():
    """each way of getting ONE rule of the step wrong moves the centres far above anything fp32 arithmetic could hide"""
    x, init = _case()
    live = torch.ones(M, dtype=torch.bool)
    live[M - 40:] = False  # the dead rows of every batch: noise around other blobs, so counting them shows
    init_e = init.clone()
    init_e[5] = 100.0  # a centre nobody is near: empty in every step
    lines = ["KMeans: what a step that gets ONE rule wrong does to the centres after three partial_fit steps (tests/kmeans_ref.py, fp64,",
             f"M {M} x 3, D {D}, K {K}, the last 40 rows of every batch dead, centre 5 far from every row); movement = max |delta c|", ""]
    good = _run_minibatch(x, init_e, live=live)[0]
    assert torch.equal(good[5], init_e[5])  # the empty centre stayed
    moved = {}
    for f in KR.FAULTS:
        moved[f] = float((_run_minibatch(x, init_e, fault=f, live=live)[0] - good).abs().max())
        lines.append(f"PARITY fault {f:<20} moves the centres by {moved[f]:.3e}")
    c = init_e.clone()
    lloyd_good = KR.lloyd_step(x[:M], c, live=live)[0]
    for f in ("dead_counted", "empty_zeroed", "mean_over_N"):
        moved["lloyd_" + f] = float((KR.lloyd_step(x[:M], c, live=live, fault=f)[0] - lloyd_good).abs().max())
        lines.append(f"PARITY fault lloyd {f:<14} moves the centres by {moved['lloyd_' + f]:.3e}")
    text = "\n".join(lines) + "\n"
    print(text)
    try:
        with open(os.path.join(ROOT, "profiles", "kmeans_faults.txt"), "w") as fh:
            fh.write(text)
    except OSError:
        pass  # a read-only checkout: the figures are in the output above
    for f, v in moved.items():
        assert v > 1e-3, (f, v)  # fp32 resolves 1e-6 of these centres


def test_dead_rows_take_no_part():
    x, init = _case()
    live = KR.live_rows([M - 40], M)
    noisy = x[:M].clone()
    noisy[M - 40:] = float("nan")
    a = KR.minibatch_step(noisy, init, torch.zeros(K, dtype=torch.int64), live=live)
    b = KR.minibatch_step(x[:M - 40], init, torch.zeros(K, dtype=torch.int64))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3] == b[3]
    assert bool((a[2][M - 40:] == K).all())


# ------------------------------------------------------------------------------------------------ the search contract's teeth
@pytest.mark.parametrize("Mp,Dp,Kp,seed", KR.PLANTED)
def test_one_fp16_rounding_fails_the_search_contract(Mp, Dp, Kp, seed):
    """the planted near-ties of tests/test_kmeans_gpu.py: an fp32-class search passes, ONE rounding of the operands to fp16 does not"""
    x, c = KR.planted(Mp, Dp, Kp, seed)
    res = KR.check_search(x, c, KR.search_emulated(x, c, "fp32"))
    assert res["violations"] == 0 and res["forced_wrong"] == 0 and res["forced"] == Mp, res
    res = KR.check_search(x, c, KR.search_emulated(x, c, "fp16"))
    print(f"planted D {Dp} K {Kp}, single fp16: {res}")
    assert res["violations"] > 0 and res["worst"] > 1.0, res


def test_plusplus_restatement():
    x, _, which = KR.blobs(64, 8, 8, spread=0.01, seed=3, scale=10.0)
    u = torch.rand(8, generator=torch.Generator().manual_seed(4))
    idx = KR.plusplus(x, 8, u)
    assert len(set(idx)) == 8 and sorted(int(which[i]) for i in idx) == list(range(8))  # one row per blob
    live = KR.live_rows([5, 0, 9, 16], 16)
    idx = KR.plusplus(x, 8, u, live=live)
    assert all(bool(live[i]) for i in idx) and len(set(idx)) == 8
    same = torch.ones(12, 8)
    assert KR.plusplus(same, 3, [0.0, 0.5, 0.99]) == [0, 6, 11]  # sum(p) == 0: floor(u M_live)


# ------------------------------------------------------------------------------------------------ host logic
@pytest.mark.parametrize("kw", [dict(n_clusters=8, dim=12), dict(n_clusters=8, dim=2056), dict(n_clusters=8, dim=4),
                                dict(n_clusters=0, dim=16), dict(n_clusters=4097, dim=16)])
def test_limits_raise_before_any_launch(kw):
    with pytest.raises(NotImplementedError, match="dim must be a multiple of 8 up to 2048|n_clusters must be in 1 .. 4096"):
        KMeans(**kw)
    with pytest.raises(NotImplementedError, match="dim must be a multiple of 8 up to 2048|n_clusters must be in 1 .. 4096"):
        kmeans_plusplus(torch.zeros(5000, kw["dim"]), kw["n_clusters"])


def test_init_variants_are_checked():
    with pytest.raises(ValueError, match='init must be "k-means\\+\\+", "random" or a tensor'):
        KMeans(4, 16, init="kmeans||")
    with pytest.raises(ValueError, match=r"init must be a float tensor \[4, 16\]"):
        KMeans(4, 16, init=torch.zeros(4, 8))
    with pytest.raises(ValueError, match=r"init must be a float tensor \[4, 16\]"):
        KMeans(4, 16, init=torch.zeros(4, 16, dtype=torch.int64))
    km = KMeans(4, 16, init=torch.ones(4, 16, dtype=torch.float64))
    assert km.cluster_centers_.dtype == torch.float32 and km.init == "array" and km.n_steps_ == 0
    assert KMeans(4, 16, init="random").init == "random" and KMeans(4, 16).init == "k-means++"


def test_lens_and_shapes_are_validated_on_the_host():
    km = KMeans(4, 16)
    f = torch.zeros(2, 10, 16)
    with pytest.raises(ValueError, match=r"features must be a tensor \[\.\., 16\]"):
        km.partial_fit(torch.zeros(5, 8))
    with pytest.raises(ValueError, match=r"KMeans: lens\[1\] = 11 is outside 0 \.\. T = 10"):
        km.partial_fit(f, lens=[3, 11])
    with pytest.raises(ValueError, match=r"KMeans: lens\[0\] = -1 is outside 0 \.\. T = 10"):
        km.fit(f, lens=torch.tensor([-1, 4]))
    with pytest.raises(ValueError, match="one entry per batch row"):
        km.partial_fit(f, lens=[3])
    with pytest.raises(ValueError, match="lens must hold ints"):
        km.partial_fit(f, lens=[3.0, 4.0])
    with pytest.raises(ValueError, match=r"needs features \[B, N, 16\]"):
        km.partial_fit(torch.zeros(20, 16), lens=[3, 4])
    with pytest.raises(ValueError, match="3 live rows cannot initialise 4 clusters"):
        km.partial_fit(f, lens=[3, 0])
    with pytest.raises(ValueError, match="3 live rows cannot initialise 4 clusters"):
        km.fit(torch.zeros(3, 16))
    with pytest.raises(ValueError, match="n_iter must be a positive int"):
        km.fit(f, n_iter=0)
    with pytest.raises(ValueError, match="predict before"):
        km.predict(f)
    with pytest.raises(ValueError, match="3 live rows cannot initialise 4 clusters"):
        kmeans_plusplus(f, 4, lens=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match=r"u must be 4 floats in \[0, 1\)"):
        kmeans_plusplus(f, 4, u=torch.zeros(3))
    with pytest.raises(ValueError, match=r"u must lie in \[0, 1\)"):
        kmeans_plusplus(f, 4, u=torch.tensor([0.0, 0.5, 1.0, 0.2]))
    with pytest.raises(ValueError, match="u and seed both given"):
        kmeans_plusplus(f, 4, u=torch.zeros(4), seed=1)


def test_cpu_tensors_raise_vbx_error():
    km = KMeans(4, 16, init=torch.zeros(4, 16))
    f = torch.zeros(2, 10, 16)
    for call in (lambda: km.partial_fit(f), lambda: km.partial_fit(f, lens=[10, 4]), lambda: km.fit(f, n_iter=2), lambda: km.predict(f),
                 lambda: kmeans_plusplus(f, 4, seed=0), lambda: KMeans(4, 16).partial_fit(f)):
        with pytest.raises(VbxError, match="runs only on an MI355X"):
            call()
    assert km.n_steps_ == 0


def test_save_is_what_load_kmeans_reads(tmp_path):
    c = torch.randn(6, 16, generator=torch.Generator().manual_seed(1))
    km = KMeans(6, 16, init=c)
    km.save(tmp_path / "km.pt")
    assert torch.equal(load_kmeans(tmp_path / "km.pt"), c)
    sd = km.state_dict()
    assert set(sd) == {"cluster_centers", "counts", "inertia", "n_steps"}
    sd["counts"], sd["n_steps"] = torch.arange(6), 3
    other = KMeans(6, 16).load_state_dict(sd)
    assert torch.equal(other.cluster_centers_, c) and torch.equal(other.counts_, torch.arange(6)) and other.n_steps_ == 3
    with pytest.raises(ValueError, match=r"cluster centres must be \[5, 16\]"):
        KMeans(5, 16).load_state_dict(sd)
    with pytest.raises(ValueError, match="nothing to save"):
        KMeans(6, 16).save(tmp_path / "none.pt")


def test_fit_kmeans_host_side():
    import hubert_ref as R

    tok = vbx.HubertWithKmeans(**R.SMALL, output_layer=2, codebook_size=64)
    with pytest.raises(NotImplementedError, match="codebook_size must be in 2 .. 4096"):
        tok.fit_kmeans([], n_clusters=1)
    with pytest.raises(ValueError, match="needs at least one batch"):
        tok.fit_kmeans([])
    with pytest.raises(ValueError, match='init must be "k-means'):
        tok.fit_kmeans([], init="nope")
    with pytest.raises(VbxError):
        tok.fit_kmeans([torch.zeros(2, 4000)])
    assert tok.codebook_size == 64


def test_entry_points_refuse_limits_before_any_launch():
    from voicebox_pytorch_amd import _lib

    l = _lib.lib()
    assert l.vbx_kmeans_search_tile(768) == 32 and l.vbx_kmeans_search_tile(1024) == 32 and l.vbx_kmeans_search_tile(1032) == 16
    assert l.vbx_kmeans_search_chunk(768) == 32 and l.vbx_kmeans_search_chunk(1024) == 16 and l.vbx_kmeans_search_chunk(2048) == 16
    assert l.vbx_kmeans_accumulate_scratch_bytes(10000, 768, 500) > 0 and l.vbx_kmeans_accumulate_scratch_bytes(10, 12, 4) == -1
    assert l.vbx_kmeans_plusplus_blocks(65) == 2
    one = 4096  # any non-null address: nothing is launched
    for name, args, msg in (("vbx_kmeans_norms", (one, one, 4, 12, None), "D must be a multiple of 8"),
                            ("vbx_kmeans_search", (one, one, one, None, one, one, 10, 10, 16, 4097, None), "K must be in 1 .. 4096"),
                            ("vbx_kmeans_search", (one, one, one, None, one, one, 10, 3, 16, 4, None), "rows must be B \\* N"),
                            ("vbx_kmeans_accumulate", (one, one, one, one, one, one, one, one, 1 << 31, 16, 4, None), "rows < 2\\^31"),
                            ("vbx_kmeans_update", (one, one, one, one, 8192, 8192, 4, 2056, 0, None), "D must be a multiple of 8"),
                            ("vbx_kmeans_update", (one, one, one, one, one, 8192, 4, 16, 0, None), "buffers of their own"),
                            ("vbx_kmeans_plusplus", (one, None, one, one, one, one, one, 10, 10, 16, 0, None), "K must be in 1 .. 4096")):
        with pytest.raises(VbxError, match=msg):
            _lib.call(name, *args)
