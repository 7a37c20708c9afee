"""Times of sample(lens=, pack=True) on one MI355X against the padded calls, by the method of tools/sample_lens_times.py:
    python tools/sample_pack_times.py [OUT.json]      (default: profiles/sample_pack_times.json)
    python tools/sample_pack_times.py --only P        (three calls of one arm and nothing else: the program of a rocprofv3
                                                       --kernel-trace --stats run, summarised by tools/prof_summary.py)

Shape: dim 512, depth 12, heads 16, 8 x 1024, 64 midpoint intervals (steps 65), lens spread evenly from 410 to 1024.  Arms alternate
in one process, window by window:

    A      sample() at the full padded shape, lens=None: wrong on the padding, the time to beat
    C      sample(lens=): the masked path (vbx_attn_fwd_lens), every padding row through every GEMM
    P      sample(lens=, pack=True): one packed row stream
    Pb     the same with pack_bucket=1024
    Pfull  pack=True with every row full (lens = N): packing can only cost here; reported against A

A window is CALLS back-to-back calls between two host synchronisations, wall clock, host side included (for P that includes
pack_rows / unpack_rows and the table refresh); the figure is the minimum of five windows per call, every window is kept so that the
spread of an arm can be read, and the three row counts of each packed arm are recorded."""
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


def main():
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    if only:
        del args[args.index("--only"):args.index("--only") + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "sample_pack_times.json")
    torch.manual_seed(0)
    vb = vbx.VoiceBox(num_cond_tokens=10, depth=MODEL["depth"], dim=MODEL["dim"], dim_head=64, heads=MODEL["heads"],
                      condition_on_text=False).to(dev).eval()
    cond = torch.randn(B, N, MODEL["dim"], device=dev)
    names = ("A", "C", "P", "Pb", "Pfull")
    wraps = {n: vbx.ConditionalFlowMatcherWrapper(voicebox=vb) for n in names}  # one sampler cache per arm
    arms = {
        "A": lambda: wraps["A"].sample(cond=cond, steps=STEPS),
        "C": lambda: wraps["C"].sample(cond=cond, steps=STEPS, lens=LENS),
        "P": lambda: wraps["P"].sample(cond=cond, steps=STEPS, lens=LENS, pack=True),
        "Pb": lambda: wraps["Pb"].sample(cond=cond, steps=STEPS, lens=LENS, pack=True, pack_bucket=1024),
        "Pfull": lambda: wraps["Pfull"].sample(cond=cond, steps=STEPS, lens=[N] * B, pack=True),
    }
    if only:  # the program of a profiler run: CALLS calls of one arm, the first one's warm-up and capture included
        for _ in range(CALLS):
            arms[only]()
        torch.cuda.synchronize()
        return
    rows = {}
    for n, fn in arms.items():  # warm up: engines, weight packing, capture
        fn()
        fn()
        s = wraps[n].last_sample_stats
        if "packed_rows" in s:
            rows[n] = {k: s[k] for k in ("packed_rows", "live_rows", "padded_rows")}
    wins = {n: [] for n in arms}
    for _ in range(WINDOWS):
        for n, fn in arms.items():  # the arms alternate
            wins[n].append(window(fn))
    row = {n: dict({"ms": round(min(w), 3), "windows": [round(x, 3) for x in w], "spread": round(max(w) - min(w), 3)}, **rows.get(n, {}))
           for n, w in wins.items()}
    for n in row:
        if n != "A":
            row[n]["ratio_to_A"] = round(row[n]["ms"] / row["A"]["ms"], 4)
        if n in ("P", "Pb"):
            row[n]["ratio_to_C"] = round(row[n]["ms"] / row["C"]["ms"], 4)
    res = {"unit": "ms per sample() call, min of %d windows of %d back-to-back calls, host side included" % (WINDOWS, CALLS),
           "shape": dict(MODEL, B=B, N=N, steps=STEPS, lens=LENS), "arms": row}
    print(json.dumps(res), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
