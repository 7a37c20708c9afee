"""Times of one KMeans.partial_fit step on one MI355X beside the same arithmetic written with torch on the device:
    python tools/kmeans_times.py [OUT.json]                                   (default: profiles/kmeans_times.json)
    python tools/kmeans_times.py --profile NAME        (7 native steps at shape NAME and nothing else: the program of a rocprofv3
                                                        --kernel-trace --stats run, profiles/kmeans_kernel_stats.txt)

    native  km.partial_fit(x[, lens=]): vbx_kmeans_norms, _search, _accumulate (six launches), _update -- csrc/kmeans.hip
    torch   fp32 on the device: |x|^2 - 2 x c^T + |c|^2 by matmul, min / argmin, index_add_, bincount, the update; under lens the live
            rows are gathered first (x[live]), as a user without lens= would
    search  vbx_kmeans_norms + vbx_kmeans_search alone: TFLOP/s = 2 M_live K D / time, beside the 157 TFLOP/s fp32 matrix peak and the
            80 TFLOP/s of vbx_rvq_encode at D 128 (profiles/codec_times.json)
    sklearn (report only, first shape) MiniBatchKMeans.partial_fit on the host, the device-to-host copy of the batch included

Shapes: 10 000 x 768 with K 500 (fairseq's learn_kmeans batch); 8 x 511 x 768 with K 500, lens spread over 40 .. 100 %; 100 000 x 1024 with
K 2000.  Arms alternate in one process, window by window.  A window is CALLS back-to-back calls between two host synchronisations, wall
clock, host side included; the figure is the minimum of WINDOWS windows per call, every window is kept and max - min of an arm's
windows stands beside it."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import torch  # noqa: E402
import voicebox_pytorch_amd as vbx  # noqa: E402
from voicebox_pytorch_amd import _lib  # noqa: E402

dev = "cuda"
WINDOWS = 5
SHAPES = [("fairseq_batch", (10000, 768), 500, None, 20), ("ragged_8x511", (8, 511, 768), 500, "spread", 20),
          ("large", (100000, 1024), 2000, None, 5)]


def window(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def measure(arms, calls, warm=3):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    wins = {n: [] for n in arms}
    for _ in range(WINDOWS):
        for n, fn in arms.items():  # the arms alternate
            wins[n].append(window(fn, calls))
    return {n: {"ms": round(min(w), 4), "windows": [round(x, 4) for x in w], "spread": round(max(w) - min(w), 4)} for n, w in wins.items()}


class TorchStep:
    """the restatement's step in fp32 with torch's own kernels"""

    def __init__(self, c):
        self.c, self.w = c.clone(), torch.zeros(c.shape[0], dtype=torch.int64, device=c.device)

    def __call__(self, x, live=None):
        x = x.reshape(-1, x.shape[-1])
        if live is not None:
            x = x[live]
        c, K = self.c, self.c.shape[0]
        d = (x * x).sum(1, keepdim=True) - 2.0 * (x @ c.t()) + (c * c).sum(1)[None, :]
        dmin, ids = d.min(dim=1)
        S = torch.zeros_like(c).index_add_(0, ids, x)
        n = torch.bincount(ids, minlength=K)
        wn = self.w + n
        self.c = torch.where((n > 0)[:, None], (c * self.w[:, None].float() + S) / wn.clamp(min=1)[:, None].float(), c)
        self.w, self.inertia = wn, dmin.sum()


def profile(which):
    name, shape, K, _, _ = [s for s in SHAPES if s[0] == which][0]
    x = torch.randn(*shape, device=dev)
    km = vbx.KMeans(K, shape[-1], init=x.reshape(-1, shape[-1])[:K].clone())
    for _ in range(7):
        km.partial_fit(x)
    torch.cuda.synchronize()


def main():
    if "--profile" in sys.argv:
        return profile(sys.argv[sys.argv.index("--profile") + 1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "kmeans_times.json")
    res = {"unit": "ms per partial_fit step, min of %d windows of back-to-back calls, host side included" % WINDOWS, "shapes": {}}
    for name, shape, K, lens_kind, calls in SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        D = shape[-1]
        x = torch.randn(*shape, device=dev, generator=g)
        init = x.reshape(-1, D)[torch.randperm(x.numel() // D, device=dev, generator=g)[:K]].clone()
        lens = live = None
        rows = x.numel() // D
        if lens_kind:
            B, N = shape[0], shape[1]
            lens_list = [round(N * (0.4 + 0.6 * i / (B - 1))) for i in range(B)]
            lens = torch.tensor(lens_list, dtype=torch.int32, device=dev)
            live = (torch.arange(N, device=dev)[None, :] < lens[:, None]).reshape(-1)
            rows = sum(lens_list)
        km, ts = vbx.KMeans(K, D, init=init), TorchStep(init)
        norms = torch.empty(K, device=dev)
        ids, mind = torch.empty(x.numel() // D, dtype=torch.int32, device=dev), torch.empty(x.numel() // D, device=dev)
        N_arg = shape[1] if lens_kind else x.numel() // D

        def search():
            st = _lib.current_stream()
            _lib.call("vbx_kmeans_norms", init, norms, K, D, st)
            _lib.call("vbx_kmeans_search", x, init, norms, lens, ids, mind, x.numel() // D, N_arg, D, K, st)

        arms = {"native": lambda: km.partial_fit(x, lens=lens), "torch": lambda: ts(x, live), "search": search}
        row = measure(arms, calls)
        row["native"]["ratio_to_torch"] = round(row["native"]["ms"] / row["torch"]["ms"], 4)
        row["native"]["faster_than_torch_by_more_than_spread"] = bool(
            row["torch"]["ms"] - row["native"]["ms"] > max(row["torch"]["spread"], row["native"]["spread"]))
        tf = 2.0 * rows * K * D / (row["search"]["ms"] * 1e-3) / 1e12
        row["search"].update(tflops=round(tf, 2), of_fp32_matrix_peak_157=round(tf / 157.0, 4), of_rvq_encode_80_at_D128=round(tf / 80.0, 4))
        entry = dict(shape=list(shape), K=K, live_rows=rows, calls_per_window=calls, arms=row)
        if name == "fairseq_batch":
            try:
                from sklearn.cluster import MiniBatchKMeans

                mb = MiniBatchKMeans(n_clusters=K, init=init.cpu().numpy(), n_init=1, reassignment_ratio=0.0, batch_size=shape[0])
                t = []
                for _ in range(4):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    mb.partial_fit(x.cpu().numpy())
                    t.append((time.perf_counter() - t0) * 1e3)
                entry["sklearn_partial_fit_host_ms_report_only"] = {"ms": round(min(t[1:]), 3), "calls": [round(v, 3) for v in t]}
            except ImportError:
                entry["sklearn_partial_fit_host_ms_report_only"] = "sklearn is not installed here"
        res["shapes"][name] = entry
        print(json.dumps({name: entry}), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
