"""Times of the train step on a ragged batch given by lengths (TrainStep.step(lens=)) on one MI355X against the masked step:
    python tools/train_lens_times.py [OUT.json] [--arms a,b,c,bfull]     (default: profiles/train_lens_times.json, all arms)
    python tools/train_lens_times.py --only b     (STEPS steps of one arm and nothing else: the program of a rocprofv3
                                                   --kernel-trace --stats run, summarised by tools/prof_summary.py)

Shape: dim 512, depth 12, heads 16, 8 x 1024 frames, lengths spread evenly from 410 to 1024 (the spread of profiles/sample_pack_times.json).
Arms alternate in one process, window by window, on one model and one TrainStep:

    a      step(x1, mask=prefix mask): the padding-mask path, every attention launch walks all key and query tiles
    b      step(x1, lens=lengths): vbx_attn_fwd_lens / vbx_attn_bwd_fused_lens stop at each row's length
    c      step(x1): all rows full, no mask (what a batch without padding costs)
    bfull  step(x1, lens=[N] * B): lengths that mask nothing; can only cost against c

A window is STEPS back-to-back steps between two host synchronisations, wall clock, host side included; the figure is the minimum of
WINDOWS windows per step, every window is kept and max - min of an arm's windows stands beside it.  `--arms a,c` runs on a tree that
has no lens= (the parent commit's arm a)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voicebox_pytorch_amd as vbx  # noqa: E402
from voicebox_pytorch_amd.dp import TrainStep  # noqa: E402

dev = "cuda"
MODEL = dict(dim=512, depth=12, heads=16, dim_head=64)
B, N = 8, 1024
LENS = [round(410 + i * (1024 - 410) / (B - 1)) for i in range(B)]
STEPS, WINDOWS = 10, 5


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / STEPS * 1e3


def take(args, flag):
    if flag not in args:
        return None
    i = args.index(flag)
    v = args[i + 1]
    del args[i:i + 2]
    return v


def main():
    args = sys.argv[1:]
    only, chosen = take(args, "--only"), take(args, "--arms")
    out = args[0] if args else os.path.join(ROOT, "profiles", "train_lens_times.json")
    torch.manual_seed(0)
    vb = vbx.VoiceBox(num_cond_tokens=10, depth=MODEL["depth"], dim=MODEL["dim"], dim_head=64, heads=MODEL["heads"],
                      condition_on_text=False).to(dev)
    ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb), lr=1e-5, max_grad_norm=0.5)
    x1 = torch.randn(B, N, MODEL["dim"], device=dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)  # a device tensor: no host read in the step
    full = torch.full((B,), N, dtype=torch.int32, device=dev)
    mask = (torch.arange(N, device=dev)[None] < lens[:, None]).contiguous()
    arms = {
        "a": lambda: ts.step(x1, mask=mask),
        "b": lambda: ts.step(x1, lens=lens),
        "c": lambda: ts.step(x1),
        "bfull": lambda: ts.step(x1, lens=full),
    }
    if only:  # the program of a profiler run
        for _ in range(STEPS):
            arms[only]()
        torch.cuda.synchronize()
        return
    if chosen:
        arms = {n: arms[n] for n in chosen.split(",")}
    for fn in arms.values():  # warm up: engine, weight packing, side stream
        for _ in range(3):
            fn()
    wins = {n: [] for n in arms}
    for _ in range(WINDOWS):
        for n, fn in arms.items():  # the arms alternate
            wins[n].append(window(fn))
    row = {n: {"ms": round(min(w), 3), "windows": [round(x, 3) for x in w], "spread": round(max(w) - min(w), 3)} for n, w in wins.items()}
    if "a" in row and "b" in row:
        row["b"]["ratio_to_a"] = round(row["b"]["ms"] / row["a"]["ms"], 4)
    if "c" in row:
        for n in ("a", "b", "bfull"):
            if n in row:
                row[n]["ratio_to_c"] = round(row[n]["ms"] / row["c"]["ms"], 4)
    res = {"unit": "ms per train step, min of %d windows of %d back-to-back steps, host side included" % (WINDOWS, STEPS),
           "shape": dict(MODEL, B=B, N=N, lens=LENS), "arms": row}
    print(json.dumps(res), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
