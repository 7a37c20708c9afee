"""Step times of the EMA kept inside the Adam launches -> profiles/ema_times.json.

Shape: dim 512 / depth 12 / heads 16, 8 x 1024 frames (bench.py's model).  Arms, alternating window by window in ONE process:
  plain  TrainStep(ema_decay=None): the train step as it was;
  fused  TrainStep(ema_decay=0.9999): every Adam launch takes its _ema entry point;
  lerp   the plain step followed by torch._foreach_lerp_ over the parameter list (what a hand-written EMA costs: a second pass over
         every fp32 parameter, 12 B each, plus its launches).
Five windows of ten steps per arm (device synchronise around each window); reported: the minimum window and max - min of the windows,
in ms per step.  Also one `with step.ema_weights():` enter + exit of the fused arm, each followed by the repack of the training engine's
operand copies that it triggers (min of five, ms).

  python tools/ema_times.py                          this tree, three arms
  python tools/ema_times.py --parent-root DIR        also the plain step of another checkout (the parent commit, built in DIR) in child
                                                     processes before and after this tree's run, same machine, same session; says
                                                     whether this tree's plain arm lies within the larger window spread of the two
  python tools/ema_times.py --arms fused --windows 1 --steps 10 --no-write       (what a rocprofv3 --kernel-trace run wraps)
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DECAY = 0.9999


def measure(root, arms, windows, steps, warmup):
    sys.path.insert(0, root)
    import torch
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep

    assert torch.cuda.is_available(), "ema_times.py measures on an MI355X; there is nothing to measure without one"
    dev = "cuda:0"
    B, N, D = 8, 1024, 512

    def model():
        torch.manual_seed(0)
        vb = vbx.VoiceBox(dim=D, num_cond_tokens=500, depth=12, dim_head=64, heads=16, condition_on_text=False)
        with torch.no_grad():
            for name, p in vb.named_parameters():
                if ".to_gamma.weight" in name or ".to_beta." in name:
                    p.normal_(0.0, 0.02)
        vb = vb.to(dev)
        return vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)

    runs, after = {}, {}
    for arm in arms:
        vb, w = model()
        runs[arm] = TrainStep(w, lr=3e-4, max_grad_norm=0.5, **(dict(ema_decay=DECAY) if arm == "fused" else {}))
        after[arm] = lambda: None
        if arm == "lerp":
            params = [p.data for p in vb.parameters()]
            avg = [p.clone() for p in params]
            after[arm] = lambda avg=avg, params=params: torch._foreach_lerp_(avg, params, 1.0 - DECAY)
    x1 = torch.randn(B, N, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for arm, ts in runs.items():
        for _ in range(warmup):
            ts.step(x1)
            after[arm]()
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for _ in range(windows):
        for arm in arms:  # alternating: a drift of the machine lands on every arm alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                runs[arm].step(x1)
                after[arm]()
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) / steps * 1e3)
    res = {arm: dict(windows_ms=[round(t, 4) for t in ts], min_ms=round(min(ts), 4), spread_ms=round(max(ts) - min(ts), 4))
           for arm, ts in times.items()}
    if "fused" in runs:  # enter + repack + exit + repack
        ts, swaps = runs["fused"], []
        eng = ts._last_eng
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ts.ema_weights():
                eng.bind_params()
            eng.bind_params()
            torch.cuda.synchronize()
            swaps.append((time.perf_counter() - t0) * 1e3)
        res["ema_weights_enter_exit"] = dict(ms=[round(t, 4) for t in swaps], min_ms=round(min(swaps), 4),
                                             what="vbx_swap_f32 + repack of the training engine's operand copies, twice")
    return res


def child(root, arms, windows, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--arms", ",".join(arms), "--windows", str(windows),
           "--steps", str(steps), "--warmup", str(warmup)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="plain,fused,lerp")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_times.json"))
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    if args.child or not args.parent_root:
        res = measure(os.path.abspath(args.root), arms, args.windows, args.steps, args.warmup)
    if args.child:
        print(json.dumps(res))
        return
    out = dict(shape="dim 512 / depth 12 / heads 16, batch 8 x 1024 frames", ema_decay=DECAY, steps_per_window=args.steps,
               windows=args.windows, unit="ms per step; min over the windows, spread = max - min of the windows")
    if args.parent_root:  # every measurement in a child process of its own, one after the other: parent, this tree, parent
        before = child(os.path.abspath(args.parent_root), ["plain"], args.windows, args.steps, args.warmup)["plain"]
        res = child(ROOT, arms, args.windows, args.steps, args.warmup)
        after = child(os.path.abspath(args.parent_root), ["plain"], args.windows, args.steps, args.warmup)["plain"]
        pw = before["windows_ms"] + after["windows_ms"]
        out["parent_plain"] = dict(windows_ms_before=before["windows_ms"], windows_ms_after=after["windows_ms"], min_ms=min(pw),
                                   spread_ms=round(max(pw) - min(pw), 4))
        if "plain" in res:
            larger = max(out["parent_plain"]["spread_ms"], res["plain"]["spread_ms"])
            out["plain_within_larger_spread_of_parent"] = bool(abs(res["plain"]["min_ms"] - min(pw)) <= larger)
    out["arms"] = res
    if "fused" in res and "lerp" in res and "plain" in res:
        spread = max(res[a]["spread_ms"] for a in ("plain", "fused", "lerp"))
        out["fused_minus_plain_ms"] = round(res["fused"]["min_ms"] - res["plain"]["min_ms"], 4)
        out["lerp_minus_plain_ms"] = round(res["lerp"]["min_ms"] - res["plain"]["min_ms"], 4)
        out["fused_beats_lerp_by_more_than_the_spread"] = bool(res["lerp"]["min_ms"] - res["fused"]["min_ms"] > spread)
    print(json.dumps(out, indent=1))
    if not args.no_write:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
