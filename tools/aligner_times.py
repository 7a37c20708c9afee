"""Times of the Aligner on one MI355X against the same network in eager PyTorch:
    python tools/aligner_times.py [OUT.json]        (default: profiles/aligner_times.json)

Three arms alternate in one process, window by window: this package's Aligner; the same network from F.conv1d with the broadcast
difference (q[:, :, :, None] - k[:, :, None]) ** 2 in fp32, which writes the B x A x T x K tensor; the same with torch.cdist(q, k) ** 2.
Per shape and arm: forward, forward + backward (ForwardSumLoss on attn_logprob plus a term on attn, parameters and inputs
differentiated) and align (forward under no_grad + maximum_path; the torch arms use this package's maximum_path and forward-sum
loss too).  A window is 10 back-to-back calls between two host synchronisations, wall clock, host side included; the figure is
the minimum of five windows per call."""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voicebox_pytorch_amd as vbx  # noqa: E402

dev = "cuda"
SHAPES = [(8, 1024, 200), (1, 301, 60)]  # B, T (mel frames), K (phonemes)
DIMS = dict(dim_in=80, dim_hidden=512, attn_channels=80)
CALLS, WINDOWS = 10, 5


def torch_forward(mod, queries, keys, mask, form):
    kl, ql = mod.key_layers, mod.query_layers
    k = F.conv1d(F.relu(F.conv1d(keys.transpose(1, 2), kl[0].weight, kl[0].bias, padding=1)), kl[2].weight, kl[2].bias)
    q = F.relu(F.conv1d(queries, ql[0].weight, ql[0].bias, padding=1))
    q = F.conv1d(F.relu(F.conv1d(q, ql[2].weight, ql[2].bias)), ql[4].weight, ql[4].bias)
    if form == "broadcast":
        d = ((q[:, :, :, None] - k[:, :, None]) ** 2).sum(1, keepdim=True)
    else:
        d = (torch.cdist(q.transpose(1, 2), k.transpose(1, 2)) ** 2)[:, None]
    logprob = -mod.temperature * d
    attn = logprob.masked_fill(~mask[:, None, None, :], -torch.finfo(logprob.dtype).max).softmax(3)
    return attn, logprob


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / CALLS * 1e3


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "aligner_times.json")
    torch.manual_seed(0)
    res = {"unit": "ms per call, min of %d windows of %d back-to-back calls, host side included" % (WINDOWS, CALLS), "dims": DIMS}
    fsl = vbx.ForwardSumLoss()
    for B, T, K in SHAPES:
        mod = vbx.Aligner(**DIMS).to(dev)
        queries = torch.randn(B, DIMS["dim_in"], T, device=dev, requires_grad=True)
        keys = torch.randn(B, K, DIMS["dim_hidden"], device=dev, requires_grad=True)
        kl = torch.full((B,), K, device=dev, dtype=torch.int64)
        kl[B // 2:] = (3 * K) // 4
        ql = torch.full((B,), T, device=dev, dtype=torch.int64)
        mask = torch.arange(K, device=dev)[None] < kl[:, None]
        arms = {"package": lambda: mod(queries, keys, mask),
                "torch_broadcast": lambda: torch_forward(mod, queries, keys, mask, "broadcast"),
                "torch_cdist": lambda: torch_forward(mod, queries, keys, mask, "cdist")}

        def fwd(arm):
            with torch.no_grad():
                arms[arm]()

        def fwd_bwd(arm):
            for p in mod.parameters():
                p.grad = None
            queries.grad = keys.grad = None
            attn, lp = arms[arm]()
            (fsl(lp, kl, ql) + attn.square().mean()).backward()

        def align(arm):
            if arm == "package":
                mod.align(queries.detach(), keys.detach(), kl, ql)
            else:
                with torch.no_grad():
                    vbx.maximum_path(arms[arm]()[0], ql, kl)

        row = {}
        for what, fn in (("forward", fwd), ("forward_backward", fwd_bwd), ("align", align)):
            for arm in arms:  # warm up: allocator, weight packing
                fn(arm)
                fn(arm)
            best = {arm: float("inf") for arm in arms}
            for _ in range(WINDOWS):
                for arm in arms:  # the arms alternate
                    best[arm] = min(best[arm], window(lambda: fn(arm)))
            row[what] = {arm: round(v, 4) for arm, v in best.items()}
        res[f"{B}x{T}x{K}"] = row
        print(f"{B}x{T}x{K}", json.dumps(row), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
