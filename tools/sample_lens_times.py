"""Times of sample(lens=) on one MI355X against the full padded call:
    python tools/sample_lens_times.py [--arms A,B,C] [--tag NAME] [OUT.json]      (default: profiles/sample_lens_times.json)

Shape: dim 512, depth 12, heads 16, 8 x 1024, 64 midpoint intervals (steps 65), lens spread evenly from 410 to 1024 (mean 70 % of
the longest).  Arms alternate in one process, window by window:

    A   sample() at the full padded shape, lens=None: wrong on the padding, the time to beat
    B   sample(lens=) with the mask only: every key tile is walked (vbx_attn_fwd)          [solver.ATTN_KEY_LENS = False]
    C   sample(lens=) with the dead key tiles skipped (vbx_attn_fwd_lens)

A window is CALLS back-to-back calls between two host synchronisations, wall clock, host side included; the figure is the minimum
of five windows per call, and every window is kept so that the spread of an arm can be read.  `--arms A` runs on a tree without
lens= (the parent commit); an existing OUT.json is updated under the --tag key, not replaced, so that the parent's A and the
branch's A, B, C land in one file.  Then the bucket effect: the first call at a new N (engine, arenas, capture) with lens alone, and
the same with length_bucket=64 after a call at another N of the same bucket."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voicebox_pytorch_amd as vbx  # noqa: E402

dev = "cuda"
MODEL = dict(dim=512, depth=12, heads=16, dim_head=64)
B, N, STEPS = 8, 1024, 65
LENS = [round(410 + i * (1024 - 410) / (B - 1)) for i in range(B)]
CALLS, WINDOWS = 3, 5


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / CALLS * 1e3


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="A,B,C")
    ap.add_argument("--tag", default="branch")
    ap.add_argument("--no-bucket", action="store_true")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "sample_lens_times.json"))
    a = ap.parse_args()
    names = a.arms.split(",")
    torch.manual_seed(0)
    vb = vbx.VoiceBox(num_cond_tokens=10, depth=MODEL["depth"], dim=MODEL["dim"], dim_head=64, heads=MODEL["heads"],
                      condition_on_text=False).to(dev).eval()
    cond = torch.randn(B, N, MODEL["dim"], device=dev)
    wraps = {n: vbx.ConditionalFlowMatcherWrapper(voicebox=vb) for n in names}  # one sampler cache per arm
    arms = {}
    if "A" in names:
        arms["A"] = lambda: wraps["A"].sample(cond=cond, steps=STEPS)
    if "B" in names or "C" in names:
        from voicebox_pytorch_amd import solver
    if "B" in names:
        arms["B"] = lambda: wraps["B"].sample(cond=cond, steps=STEPS, lens=LENS)
    if "C" in names:
        arms["C"] = lambda: wraps["C"].sample(cond=cond, steps=STEPS, lens=LENS)
    for n, fn in arms.items():  # warm up: engines, weight packing, capture (the switch is read when a sampler is built)
        if n in ("B", "C"):
            solver.ATTN_KEY_LENS = n == "C"
        fn()
        fn()
    if "B" in names or "C" in names:
        solver.ATTN_KEY_LENS = True
    wins = {n: [] for n in arms}
    for _ in range(WINDOWS):
        for n, fn in arms.items():  # the arms alternate
            wins[n].append(window(fn))
    row = {n: {"ms": round(min(w), 3), "windows": [round(x, 3) for x in w], "spread": round(max(w) - min(w), 3)} for n, w in wins.items()}
    if "A" in row:
        for n in row:
            if n != "A":
                row[n]["ratio_to_A"] = round(row[n]["ms"] / row["A"]["ms"], 4)
    print(a.tag, json.dumps(row), flush=True)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res["unit"] = "ms per sample() call, min of %d windows of %d back-to-back calls, host side included" % (WINDOWS, CALLS)
    res["shape"] = dict(MODEL, B=B, N=N, steps=STEPS, lens=LENS)
    res[a.tag] = row
    if "C" in names and not a.no_bucket:
        # the first call at a new N: 900 builds a sampler; with length_bucket=64 after a call at 930 (same bucket, 960) it does not
        w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
        c900, c930 = cond[:, :900].contiguous(), cond[:, :930].contiguous()
        l900 = [min(l, 900) for l in LENS]
        plain = once(lambda: w.sample(cond=c900, steps=STEPS, lens=l900))
        steady = once(lambda: w.sample(cond=c900, steps=STEPS, lens=l900))
        w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
        w.sample(cond=c930, steps=STEPS, lens=[min(l, 930) for l in LENS], length_bucket=64)
        bucket = once(lambda: w.sample(cond=c900, steps=STEPS, lens=l900, length_bucket=64))
        res["first_call_at_new_N_ms"] = {"lens": round(plain, 2), "lens_and_length_bucket_64": round(bucket, 2),
                                         "steady_call_at_that_N": round(steady, 2)}
        print("first call at a new N", json.dumps(res["first_call_at_new_N_ms"]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
