"""Aligner primitives: the native kernels (csrc/align.hip) beside the same arithmetic written with torch on the same device.

    python tools/align_times.py [OUT.json]            (default: profiles/align_times.json)
    python tools/align_times.py --profile B T K       (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

Two figures per shape B x T x K (full lengths, random inputs):
  maximum_path   native: vbx.maximum_path.  torch: the same dynamic programme as a T-step loop of torch ops over [B, K] rows and the
                 backtrack as a second T-step loop of gathers, all on the device (torch_path below).  Context only, one call: the
                 host round trip of the reference world, value.cpu() -> a numpy loop over the frames -> path.to(device).
  forward_sum    loss and gradient.  native: vbx.forward_sum_loss(...).backward().  torch: pad + mask + log_softmax + F.ctc_loss
                 (blank 0, zero_infinity) on the device, and its backward.

The parent runs one child process per shape under `timeout -k 10 <seconds>`; a child that fails is reported and nothing is started
after it.  In a child both arms run in one process, alternating, after warm-up, device events around windows of back-to-back calls
(the host side of a call included); the minimum of the windows is the figure."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024, 200), (1, 301, 60)]
CALLS, REPS, WARM = 10, 5, 2


def torch_path(value):
    """maximum_path at full lengths with torch ops on value's device: (path [B, T, K], durations [B, K])"""
    import torch

    B, T, K = value.shape
    ninf = torch.full((B, 1), float("-inf"), device=value.device)
    xs = torch.arange(K, device=value.device)
    rows = torch.arange(B, device=value.device)
    Q = torch.full((B, K), float("-inf"), device=value.device)
    Q[:, 0] = value[:, 0, 0]
    moves = [None]
    for y in range(1, T):
        left = torch.cat((ninf, Q[:, :-1]), 1)
        moves.append(Q < left)  # strict: a tie stays; the diagonal cell has Q = -inf and moves
        band = (xs <= y) & (xs >= K + y - T)
        Q = torch.where(band, torch.maximum(Q, left) + value[:, y], ninf)
    path = torch.zeros_like(value)
    idx = torch.full((B,), K - 1, device=value.device, dtype=torch.int64)
    for y in range(T - 1, -1, -1):
        path[rows, y, idx] = 1.0
        if y > 0:
            idx = idx - moves[y][rows, idx].to(torch.int64)
    return path, path.sum(1).to(torch.int64)


def numpy_path(value):
    """the host round trip: device -> numpy loop over the frames -> device"""
    import numpy as np
    import torch

    v = value.cpu().numpy().astype(np.float64)
    B, T, K = v.shape
    path = np.zeros((B, T, K), dtype=np.float32)
    xs = np.arange(K)
    for b in range(B):
        Q = np.full((T, K), -np.inf)
        Q[0, 0] = v[b, 0, 0]
        for y in range(1, T):
            left = np.concatenate(([-np.inf], Q[y - 1, :-1]))
            band = (xs <= y) & (xs >= K + y - T)
            Q[y] = np.where(band, np.maximum(Q[y - 1], left) + v[b, y], -np.inf)
        idx = K - 1
        for y in range(T - 1, -1, -1):
            path[b, y, idx] = 1.0
            if y > 0 and idx > 0 and Q[y - 1, idx] < Q[y - 1, idx - 1]:
                idx -= 1
    return torch.from_numpy(path).to(value.device)


def torch_forward_sum(x, blank=-1.0):
    """the loss with torch's own pieces on x's device (full lengths): returns the scalar, differentiable"""
    import torch
    import torch.nn.functional as F

    B, T, K = x.shape
    lp = torch.log_softmax(F.pad(x, (1, 0), value=blank), 2).transpose(0, 1)
    targets = torch.arange(1, K + 1, device=x.device)[None, :].expand(B, K)
    lens_t = torch.full((B,), T, device=x.device, dtype=torch.int64)
    lens_k = torch.full((B,), K, device=x.device, dtype=torch.int64)
    return F.ctc_loss(lp, targets, lens_t, lens_k, blank=0, reduction="mean", zero_infinity=True)


def setup(B, T, K):
    import torch

    sys.path.insert(0, ROOT)
    import voicebox_pytorch_amd as vbx

    g = torch.Generator().manual_seed(0)
    value = torch.randn(B, T, K, generator=g).to("cuda")
    x = (3.0 * torch.randn(B, T, K, generator=g)).to("cuda").requires_grad_(True)
    return torch, vbx, value, x


def child(B, T, K):
    torch, vbx, value, x = setup(B, T, K)

    def native_loss():
        x.grad = None
        vbx.forward_sum_loss(x).backward()
        return x.grad

    def torch_loss():
        x.grad = None
        torch_forward_sum(x).backward()
        return x.grad

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    paths = {"maximum_path": (lambda: vbx.maximum_path(value), nograd(lambda: torch_path(value))),
             "forward_sum_fwd_bwd": (native_loss, torch_loss)}
    res = {"B": B, "T": T, "K": K}
    for nat, ref in paths.values():
        for _ in range(WARM):
            nat()
            ref()
    torch.cuda.synchronize()
    times = {(k, arm): [] for k in paths for arm in ("native", "torch")}
    for _ in range(REPS):  # alternating windows
        for k, fns in paths.items():
            for arm, fn in zip(("native", "torch"), fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(CALLS):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[(k, arm)].append(a.elapsed_time(b) / CALLS)
    for k in paths:
        entry = {}
        for arm in ("native", "torch"):
            v = times[(k, arm)]
            entry[arm + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=CALLS, windows=REPS)
        entry["native_over_torch_min"] = entry["native_ms_per_call"]["min"] / entry["torch_ms_per_call"]["min"]
        res[k] = entry
    # context: the host round trip, one call, host clock around a synchronised call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = numpy_path(value)
    torch.cuda.synchronize()
    res["maximum_path"]["host_round_trip_numpy_ms_one_call"] = (time.perf_counter() - t0) * 1e3
    # the arms must agree: scores of the three paths (ties have probability zero on Gaussian scores), loss and gradient
    p_nat, d_nat = vbx.maximum_path(value)
    p_t, d_t = torch_path(value)
    res["maximum_path"]["paths_equal_native_torch"] = bool(torch.equal(p_nat, p_t)) and bool(torch.equal(d_nat, d_t))
    res["maximum_path"]["paths_equal_native_numpy"] = bool(torch.equal(p_nat, host))
    g_nat = native_loss().clone()
    l_nat = float(vbx.forward_sum_loss(x))
    g_t = torch_loss().clone()
    l_t = float(torch_forward_sum(x))
    res["forward_sum_fwd_bwd"].update(loss_native=l_nat, loss_torch=l_t, grad_max_abs_diff=float((g_nat - g_t).abs().max()),
                                      grad_max_abs=float(g_t.abs().max()))
    print("RESULT " + json.dumps(res))


def profile(B, T, K):
    torch, vbx, value, x = setup(B, T, K)
    for _ in range(WARM + CALLS):
        vbx.maximum_path(value)
        x.grad = None
        vbx.forward_sum_loss(x).backward()
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "align_times.json")
    results = {"note": f"ms per call, full lengths, random inputs; device events around {REPS} alternating windows of {CALLS} back-to-back "
                       "calls per arm in one process (host side of the call included), one MI355X; torch = the same arithmetic with "
                       "torch ops on the same device (tools/align_times.py: torch_path, torch_forward_sum); forward_sum_fwd_bwd = loss "
                       "and gradient; host_round_trip_numpy = context only, one call; produced by tools/align_times.py", "shapes": []}
    for B, T, K in SHAPES:
        cmd = ["timeout", "-k", "10", "280", sys.executable, os.path.abspath(__file__), "--child", str(B), str(T), str(K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results["shapes"].append({"B": B, "T": T, "K": K, "failed_rc": p.returncode, "stderr_tail": p.stderr[-600:]})
            break  # nothing more is started on the device after a failure
        results["shapes"].append(json.loads(line[0][7:]))
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 0 if all("failed_rc" not in s for s in results["shapes"]) else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*(int(a) for a in sys.argv[2:5]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(*(int(a) for a in sys.argv[2:5]))
    else:
        sys.exit(main())
