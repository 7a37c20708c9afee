"""KMeans / kmeans_plusplus: fitting a k-means codebook on the device (csrc/kmeans.hip) -- the cluster centres HubertWithKmeans needs
beside HuBERT's weights, from features that already sit in GPU memory (tok.features(wave, lens=)).

    km = KMeans(n_clusters=500, dim=768, init="k-means++", seed=0)
    km.partial_fit(feats, lens=frame_lens)    # ONE MiniBatchKMeans step at reassignment_ratio = 0
    km.fit(feats, n_iter=20)                  # Lloyd: n_iter full-batch steps
    ids = km.predict(feats)                   # vbx_kmeans_assign: the ids HubertWithKmeans gives with these centres

A step assigns every live row with the OLD centres (vbx_kmeans_search), sums the members of every cluster in a fixed order
(vbx_kmeans_accumulate) and moves the centres (vbx_kmeans_update): c <- (c w + sum) / (w + n), w <- w + n for partial_fit, c <- sum / n
for fit; a centre without members keeps its value.  PINNED against sklearn 1.7.2 through the fp64 restatement tests/kmeans_ref.py
(tests/test_kmeans_cpu.py: MiniBatchKMeans.partial_fit and KMeans(algorithm="lloyd") with init=array, n_init=1, on inputs without
an empty cluster).  TWO STATED DIFFERENCES: sklearn.KMeans relocates an empty centre, fit() here leaves it (counts_ shows it); and
kmeans_plusplus is the plain D^2 sampling of Arthur & Vassilvitskii with one candidate per step and its own uniforms -- sklearn's
greedy variant (2 + log K candidates) and its random stream are UNPINNED.

No entry point synchronises with the host: chosen indices, counts and inertia stay on the device.  GPU tensors only (a CPU tensor:
VbxError).  lens: a list or CPU tensor is validated (ValueError), a device tensor is clamped into 0 .. N on the device; with a device
lens that leaves fewer live rows than n_clusters the initialisation is undefined (rows repeat) but memory-safe."""
import torch

from . import _lib
from .wave_lens import device_lens

MAX_DIM, MAX_CLUSTERS, MAX_ROWS = 2048, 4096, 2 ** 31 - 1  # csrc/kmeans.hip and vbx_kmeans_assign
_INITS = ("k-means++", "random")


def _check_limits(D, K, who):
    if not isinstance(D, int) or D < 8 or D % 8 or D > MAX_DIM:
        raise NotImplementedError(f"{who}: dim must be a multiple of 8 up to {MAX_DIM} (got {D})")
    if not isinstance(K, int) or not 1 <= K <= MAX_CLUSTERS:
        raise NotImplementedError(f"{who}: n_clusters must be in 1 .. {MAX_CLUSTERS} (got {K})")


def _prepare(feats, lens, D, K_init, who):
    """-> (x fp32 contiguous [.., D], lens int32 [B] on the device or None, M rows, N rows per batch row).  Every host-side refusal
    comes first, the device check last.  K_init: the number of live rows an initialisation on this batch needs (None: no
    initialisation), checked where lens is visible on the host."""
    if not isinstance(feats, torch.Tensor) or feats.ndim < 1 or feats.shape[-1] != D:
        got = tuple(feats.shape) if isinstance(feats, torch.Tensor) else type(feats).__name__
        raise ValueError(f"{who}: features must be a tensor [.., {D}] (got {got})")
    M = feats.numel() // D
    if M < 1:
        raise ValueError(f"{who}: no rows")
    if M > MAX_ROWS:
        raise NotImplementedError(f"{who}: rows must stay below 2^31 (got {M})")
    N, live, lens_dev = M, M, None
    if lens is not None:
        if feats.ndim != 3:
            raise ValueError(f"{who}: lens counts the rows of each batch row and needs features [B, N, {D}] (got {tuple(feats.shape)})")
        B, N = feats.shape[0], feats.shape[1]
        lens_dev = device_lens(lens, B, N, 0, feats.device, who)
        host = not (torch.is_tensor(lens) and lens.device.type != "cpu")
        live = int(sum(int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens))) if host else None
    if K_init is not None and live is not None and live < K_init:
        raise ValueError(f"{who}: {live} live rows cannot initialise {K_init} clusters")
    if feats.device.type != "cuda":
        raise _lib.VbxError(f"{who} runs only on an MI355X (gfx950) through libvbx_hip.so; the features are on '{feats.device}'")
    return feats.detach().to(torch.float32).contiguous(), lens_dev, M, N


def _check_u(u, K, device, who):
    """u -> fp32 [K] on the device; host values are checked to lie in [0, 1)"""
    t = torch.as_tensor(u)
    if t.ndim != 1 or t.shape[0] != K or not t.is_floating_point():
        raise ValueError(f"{who}: u must be {K} floats in [0, 1) (got shape {tuple(t.shape)}, dtype {t.dtype})")
    if t.device.type == "cpu" and not bool(((t >= 0) & (t < 1)).all()):
        raise ValueError(f"{who}: u must lie in [0, 1)")
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _plusplus(x, lens_dev, M, N, D, K, u):
    dev = x.device
    p = torch.empty(M, dtype=torch.float32, device=dev)
    bsum = torch.empty(_lib.lib().vbx_kmeans_plusplus_blocks(M), dtype=torch.float64, device=dev)
    chosen = torch.empty(K, dtype=torch.int64, device=dev)
    centers = torch.empty(K, D, dtype=torch.float32, device=dev)
    _lib.call("vbx_kmeans_plusplus", x, lens_dev, u, p, bsum, chosen, centers, M, N, D, K, _lib.current_stream())
    return centers, chosen


def kmeans_plusplus(x, n_clusters, u=None, seed=None, lens=None):
    """Plain D^2 sampling (Arthur & Vassilvitskii 2007), one candidate per step -> (centers fp32 [K, D], indices int64 [K] into the
    rows of x flattened to [M, D]), both on the device.  u: fp32 [K] in [0, 1), drawn on the device from `seed` when not given.
    Step 0 picks live row floor(u_0 * M_live); step j the first live row whose running sum of p_i = min over the chosen rows of
    |x_i - x_c|^2 (by differences: exactly 0 for a chosen row) reaches u_j * sum(p), the running sum in fp64 in the fixed order
    include/vbx.h states; if sum(p) == 0, live row floor(u_j * M_live).  sklearn's greedy variant and its random stream are NOT
    reproduced (unpinned)."""
    who = "kmeans_plusplus"
    if not isinstance(x, torch.Tensor) or x.ndim < 1:
        raise ValueError(f"{who}: x must be a tensor [.., D]")
    D, K = int(x.shape[-1]), n_clusters
    _check_limits(D, K, who)
    if u is not None and seed is not None:
        raise ValueError(f"{who}: u and seed both given -- the uniforms are either yours or drawn from the seed")
    if u is not None:
        u = _check_u(u, K, x.device, who)
    x, lens_dev, M, N = _prepare(x, lens, D, K, who)
    if lens is None and M < K:
        raise ValueError(f"{who}: {M} live rows cannot initialise {K} clusters")
    if u is None:
        g = torch.Generator(device=x.device)
        g.manual_seed(0 if seed is None else int(seed))
        u = torch.rand(K, generator=g, device=x.device, dtype=torch.float32)
    return _plusplus(x, lens_dev, M, N, D, K, u)


class KMeans:
    """n_clusters centres of `dim` components.  init: "k-means++" | "random" | fp32 tensor [K, D]; the first two run on the first batch
    handed to partial_fit / fit, over its live rows only ("random": K distinct live rows by torch's device generator).

    cluster_centers_ fp32 [K, D]; counts_ int64 [K] (partial_fit: the weight w summed over all steps; fit: the members of the last
    iteration -- 0 marks an empty centre, which kept its value); inertia_ fp32 scalar on the device: the sum of the live rows' min
    distances of the last step, measured BEFORE its update (fp64 sum in a fixed order, rounded once); labels_ int32: the last step's
    ids (n_clusters for a dead row); n_steps_.

    Limits, refused before any launch: dim a multiple of 8 up to 2048 and n_clusters 1 .. 4096 (NotImplementedError); rows below
    2^31; fewer live rows than n_clusters at the initialisation and lens outside 0 .. N (ValueError; a device lens is clamped and
    not counted: undefined but memory-safe)."""

    def __init__(self, n_clusters, dim, init="k-means++", seed=0):
        who = "KMeans"
        _check_limits(dim, n_clusters, who)
        self.n_clusters, self.dim, self.seed = n_clusters, dim, int(seed)
        self.cluster_centers_ = self.counts_ = self.inertia_ = self.labels_ = None
        self.n_steps_ = 0
        self._scratch = None
        if isinstance(init, torch.Tensor):
            if tuple(init.shape) != (n_clusters, dim) or not init.is_floating_point():
                raise ValueError(f"{who}: init must be a float tensor [{n_clusters}, {dim}] (got {tuple(init.shape)}, {init.dtype})")
            self.init = "array"
            self.cluster_centers_ = init.detach().to(torch.float32).clone().contiguous()
        elif init in _INITS:
            self.init = init
        else:
            raise ValueError(f'{who}: init must be "k-means++", "random" or a tensor [{n_clusters}, {dim}] (got {init!r})')

    # -- state
    def state_dict(self):
        return {"cluster_centers": self.cluster_centers_, "counts": self.counts_, "inertia": self.inertia_, "n_steps": self.n_steps_}

    def load_state_dict(self, sd):
        c = torch.as_tensor(sd["cluster_centers"]).detach().to(torch.float32)
        if tuple(c.shape) != (self.n_clusters, self.dim):
            raise ValueError(f"KMeans: cluster centres must be [{self.n_clusters}, {self.dim}] (got {tuple(c.shape)})")
        self.cluster_centers_ = c.clone().contiguous()
        w = sd.get("counts")
        self.counts_ = None if w is None else torch.as_tensor(w).detach().to(device=c.device, dtype=torch.int64).clone()
        self.inertia_, self.n_steps_ = sd.get("inertia"), int(sd.get("n_steps", 0))
        return self

    def save(self, path):
        """the plain [K, D] tensor, as hubert.load_kmeans / HubertWithKmeans.from_checkpoint read it"""
        if self.cluster_centers_ is None:
            raise ValueError("KMeans: nothing to save before the first partial_fit / fit")
        torch.save(self.cluster_centers_.detach().cpu(), str(path))

    # -- steps
    def _initialise(self, x, lens_dev, M, N):
        dev, K, D = x.device, self.n_clusters, self.dim
        if self.cluster_centers_ is None:
            g = torch.Generator(device=dev)
            g.manual_seed(self.seed)
            if self.init == "k-means++":
                u = torch.rand(K, generator=g, device=dev, dtype=torch.float32)
                self.cluster_centers_ = _plusplus(x, lens_dev, M, N, D, K, u)[0]
            else:  # K distinct live rows: the K smallest of M uniforms, the dead rows' pushed past 1
                r = torch.rand(M, generator=g, device=dev, dtype=torch.float32)
                if lens_dev is not None:
                    r = r.view(-1, N).masked_fill(torch.arange(N, device=dev)[None, :] >= lens_dev[:, None], 2.0).view(M)
                self.cluster_centers_ = x.view(M, D)[torch.topk(r, K, largest=False).indices].contiguous()
        elif self.cluster_centers_.device != dev:
            self.cluster_centers_ = self.cluster_centers_.to(dev)
        if self.counts_ is None:
            self.counts_ = torch.zeros(K, dtype=torch.int64, device=dev)
        elif self.counts_.device != dev:
            self.counts_ = self.counts_.to(dev)

    def _step(self, x, lens_dev, M, N, lloyd):
        dev, K, D, st = x.device, self.n_clusters, self.dim, _lib.current_stream()
        c, w = self.cluster_centers_, self.counts_
        norms = torch.empty(K, dtype=torch.float32, device=dev)
        ids = torch.empty(M, dtype=torch.int32, device=dev)
        mind = torch.empty(M, dtype=torch.float32, device=dev)
        _lib.call("vbx_kmeans_norms", c, norms, K, D, st)
        _lib.call("vbx_kmeans_search", x, c, norms, lens_dev, ids, mind, M, N, D, K, st)
        sums, counts = self._accumulate(x, ids, mind, M)
        c_out, w_out = torch.empty_like(c), torch.empty_like(w)
        _lib.call("vbx_kmeans_update", c, w, sums, counts, c_out, w_out, K, D, 1 if lloyd else 0, st)
        self.cluster_centers_, self.counts_, self.labels_ = c_out, w_out, ids
        self.n_steps_ += 1

    def _accumulate(self, x, ids, mind, M):
        """-> (sums fp32 [K, D], counts int32 [K]); sets inertia_"""
        dev, K, D = x.device, self.n_clusters, self.dim
        need = _lib.lib().vbx_kmeans_accumulate_scratch_bytes(M, D, K)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        sums = torch.empty(K, D, dtype=torch.float32, device=dev)
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        in64, in32 = torch.empty(1, dtype=torch.float64, device=dev), torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("vbx_kmeans_accumulate", x, ids, mind, sums, counts, in64, in32, self._scratch, M, D, K, _lib.current_stream())
        self.inertia_ = in32
        return sums, counts

    @torch.no_grad()
    def partial_fit(self, feats, lens=None):
        """ONE MiniBatchKMeans step at reassignment_ratio = 0 on feats fp32 [.., D]; lens: feats [B, N, D], only rows n < lens[b] count"""
        x, lens_dev, M, N = _prepare(feats, lens, self.dim, self.n_clusters if self.cluster_centers_ is None else None, "KMeans")
        if self.cluster_centers_ is None and lens is None and M < self.n_clusters:
            raise ValueError(f"KMeans: {M} live rows cannot initialise {self.n_clusters} clusters")
        self._initialise(x, lens_dev, M, N)
        self._step(x, lens_dev, M, N, lloyd=False)
        return self

    @torch.no_grad()
    def fit(self, feats, n_iter=20, lens=None):
        """Lloyd: n_iter full-batch steps c <- mean of the members; an empty centre stays where it is (sklearn relocates it)"""
        if not isinstance(n_iter, int) or n_iter < 1:
            raise ValueError(f"KMeans: n_iter must be a positive int (got {n_iter!r})")
        x, lens_dev, M, N = _prepare(feats, lens, self.dim, self.n_clusters if self.cluster_centers_ is None else None, "KMeans")
        if self.cluster_centers_ is None and lens is None and M < self.n_clusters:
            raise ValueError(f"KMeans: {M} live rows cannot initialise {self.n_clusters} clusters")
        self._initialise(x, lens_dev, M, N)
        for _ in range(n_iter):
            self._step(x, lens_dev, M, N, lloyd=True)
        return self

    @torch.no_grad()
    def predict(self, feats):
        """vbx_kmeans_assign of feats fp32 [.., D] -> int64 [..]: what HubertWithKmeans.assign gives with these centres"""
        if self.cluster_centers_ is None:
            raise ValueError("KMeans: predict before the first partial_fit / fit")
        x, _, M, _ = _prepare(feats, None, self.dim, None, "KMeans")
        if self.cluster_centers_.device != x.device:
            self.cluster_centers_ = self.cluster_centers_.to(x.device)
        ids = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
        _lib.call("vbx_kmeans_assign", x, self.cluster_centers_, ids, M, self.dim, self.n_clusters, _lib.current_stream())
        return ids
