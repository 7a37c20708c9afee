"""Step times of fine-tuning on the device -> profiles/finetune_times.json.

Shape: dim 512 / depth 12 / heads 16, 8 x 1024 frames (bench.py's model).  Arms, alternating window by window in ONE process:
  full     the full train step (nothing frozen, no adapters);
  frozen6  the same step with the lower six layers frozen (requires_grad=False on every parameter of layers 0 .. 5);
  lora16   LoRA at rank 16 on all four targets of every layer, base frozen.
Five windows of ten steps per arm (device synchronise around each window); reported: the minimum window and max - min of the windows,
in ms per step.

  python tools/finetune_times.py                         this tree, three arms
  python tools/finetune_times.py --parent-root DIR       also the full step of another checkout (the parent commit, built in DIR) in
                                                         child processes before and after this tree's run, same machine, same session;
                                                         says whether this tree's full arm lies inside the parent's window spread
  python tools/finetune_times.py --arms lora16 --windows 1 --steps 10 --no-write      (what a rocprofv3 --kernel-trace run wraps)
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(root, arms, windows, steps, warmup):
    sys.path.insert(0, root)
    import torch
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep

    assert torch.cuda.is_available(), "finetune_times.py measures on an MI355X; there is nothing to measure without one"
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

    runs = {}
    for arm in arms:
        vb, w = model()
        if arm == "frozen6":
            for l in range(6):
                for p in vb.transformer.layers[l].parameters():
                    p.requires_grad_(False)
        elif arm == "lora16":
            vb.add_lora(rank=16, alpha=16.)
        runs[arm] = TrainStep(w, lr=3e-4, max_grad_norm=0.5)
    x1 = torch.randn(B, N, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for ts in runs.values():
        for _ in range(warmup):
            ts.step(x1)
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for _ in range(windows):
        for arm in arms:  # alternating: a drift of the machine lands on every arm alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                runs[arm].step(x1)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) / steps * 1e3)
    return {arm: dict(windows_ms=[round(t, 4) for t in ts], min_ms=round(min(ts), 4), spread_ms=round(max(ts) - min(ts), 4))
            for arm, ts in times.items()}


def child(root, arms, windows, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--arms", ",".join(arms), "--windows", str(windows),
           "--steps", str(steps), "--warmup", str(warmup)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="full,frozen6,lora16")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_times.json"))
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    if args.child or not args.parent_root:
        res = measure(os.path.abspath(args.root), arms, args.windows, args.steps, args.warmup)
    if args.child:
        print(json.dumps(res))
        return
    out = dict(shape="dim 512 / depth 12 / heads 16, batch 8 x 1024 frames", steps_per_window=args.steps, windows=args.windows,
               unit="ms per step; min over the windows, spread = max - min of the windows")
    if args.parent_root:  # every measurement in a child process of its own, one after the other: parent, this tree, parent
        before = child(os.path.abspath(args.parent_root), ["full"], args.windows, args.steps, args.warmup)["full"]
        res = child(ROOT, arms, args.windows, args.steps, args.warmup)
        after = child(os.path.abspath(args.parent_root), ["full"], args.windows, args.steps, args.warmup)["full"]
        pw = before["windows_ms"] + after["windows_ms"]
        out["parent_full"] = dict(windows_ms_before=before["windows_ms"], windows_ms_after=after["windows_ms"], min_ms=min(pw),
                                  spread_ms=round(max(pw) - min(pw), 4))
        out["full_inside_parent_spread"] = bool(res["full"]["min_ms"] <= max(pw)) if "full" in res else None
    out["arms"] = res
    print(json.dumps(out, indent=1))
    if not args.no_write:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
