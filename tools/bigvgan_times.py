"""BigVGANGenerator: the native launch sequence (csrc/bigvgan.hip) beside what a user would write without it -- the same network from
torch.nn.functional (F.conv1d, F.conv_transpose1d, F.pad(mode="replicate"), torch.sin) on the same device, in fp32 and under fp16
autocast.  Two configurations with random weights: BASE, the base published widths (100 mels, 512 channels, rates 8 8 2 2), and
WIDE, the large published shape (1536 channels, rates 4 4 2 2 2 2, clamp, no final bias).  One MI355X.

    python tools/bigvgan_times.py [OUT.json]                   (default: profiles/bigvgan_times.json)
    python tools/bigvgan_times.py --profile CONFIG B FRAMES [everywhere | nowhere]
                                                  (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

One process: per shape the arms run alternating, after warm-up, device events around windows of back-to-back calls (the host side of
a call included); the minimum of the windows is the figure, their spread is recorded.  The native path runs at its default and
twice more as the A/B behind BigVGANGenerator.FUSE_ACT_MAX_CHANNELS: with Activation1d fused into every residual convolution's staging
(vbx_bigvgan_conv) and into none (vbx_bigvgan_act + vbx_hifigan_conv); and per stage the residual convolutions alone, fused against
unfused, which is what the default is read off."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024, 3), (1, 301, 8)]  # B, frames, calls per window
REPS, WARM = 5, 2


def configs(R):
    base = dict(R.WIDE, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                use_tanh_at_final=True, use_bias_at_final=True)
    return {"BASE": base, "WIDE": R.WIDE}


def torch_generator(R, sd, cfg, dev):
    """the generator from torch's own operators on `dev`, weight norm folded and the snake parameters exponentiated once"""
    import torch
    import torch.nn.functional as F

    w = {p: R.fold(sd, p, torch.float32).to(dev) for p, *_ in R.layout(cfg)}
    b = {p: sd[f"{p}.bias"].to(dev) if f"{p}.bias" in sd else None for p, *_ in R.layout(cfg)}
    acts = {}
    for p, c in R.act_layout(cfg):
        al, ib = R.snake_params(sd, p, cfg, torch.float32)
        acts[p] = (al.to(dev), ib.to(dev), sd[f"{p}.upsample.filter"].reshape(12).to(dev), sd[f"{p}.downsample.lowpass.filter"].reshape(12).to(dev))
    nk = len(cfg["resblock_kernel_sizes"])

    def conv(x, p, d=1):
        k = w[p].shape[-1]
        return F.conv1d(x, w[p], b[p], dilation=d, padding=(k - 1) * d // 2)

    def act(x, p):
        return R.activation1d(x, *acts[p])

    def fwd(mel):
        x = conv(mel, "conv_pre")
        for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
            x = F.conv_transpose1d(x, w[f"ups.{i}.0"], b[f"ups.{i}.0"], stride=u, padding=(k - u) // 2)
            xs = None
            for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
                rb, h = f"resblocks.{i * nk + j}", x
                for m, d in enumerate(ds):
                    t = conv(act(h, f"{rb}.activations.{2 * m}"), f"{rb}.convs1.{m}", d)
                    h = conv(act(t, f"{rb}.activations.{2 * m + 1}"), f"{rb}.convs2.{m}") + h
                xs = h if xs is None else xs + h
            x = xs / nk
        x = conv(act(x, "activation_post"), "conv_post")
        return (torch.tanh(x) if cfg["use_tanh_at_final"] else torch.clamp(x, -1.0, 1.0))[:, 0]

    return fwd


def setup(name):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bigvgan_ref as R
    import voicebox_pytorch_amd as vbx

    cfg = configs(R)[name]
    sd = R.random_state(cfg, 0)
    model = vbx.BigVGANGenerator(**cfg)
    model.load_state_dict(sd, strict=True)
    return torch, R, cfg, sd, model.to("cuda").eval()


def windows(torch, paths, calls, reps):
    times = {k: [] for k in paths}
    for _ in range(reps):  # alternating windows
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return times


def summary(v, calls):
    return dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), spread=(max(v) - min(v)) / min(v), calls=calls, windows=len(v))


def with_fuse(model, width, fn):
    def run():
        default = model.fuse_act_max_channels
        model.fuse_act_max_channels = width
        try:
            return fn()
        finally:
            model.fuse_act_max_channels = default
    return run


def stage_convs(torch, model, stage, B, L, fused):
    """the residual convolutions of one stage alone on a random activation [B, L, C], their activation fused or a launch of its own"""
    ops = model.packed_ops()["stages"][stage]
    C = ops["C"] // 2
    x = torch.randn(B, L, C, generator=torch.Generator().manual_seed(stage)).half().to("cuda")

    def run():
        from voicebox_pytorch_amd import _lib

        st = _lib.current_stream()
        default = model.fuse_act_max_channels
        model.fuse_act_max_channels = None if fused else 0
        try:
            for block in ops["blocks"]:
                h = x
                for a1, c1, a2, c2 in block:
                    h = model._act_conv(a2, c2, model._act_conv(a1, c1, h, None, B, L, st), h, B, L, st)
        finally:
            model.fuse_act_max_channels = default
    return run, C


def measure(torch, R, cfg, model, ref, B, frames, calls):
    mel = R.mels(B, cfg["n_mels"], frames, 1).to("cuda")

    def fp32():
        with torch.inference_mode():
            return ref(mel)

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return ref(mel)

    paths = {"native": lambda: model(mel), "torch_fp32": fp32, "torch_fp16_autocast": autocast,
             "native_fused_everywhere": with_fuse(model, None, lambda: model(mel)), "native_fused_nowhere": with_fuse(model, 0, lambda: model(mel))}
    res = {"B": B, "frames": frames, "samples": frames * model.hop_length, "default_fuse_act_max_channels": model.fuse_act_max_channels}
    for name, fn in paths.items():
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        print(f"warmed {name} at B {B} frames {frames}", flush=True)
    for k, v in windows(torch, paths, calls, REPS).items():
        res[k + "_ms_per_call"] = summary(v, calls)
    print(f"timed the whole network at B {B} frames {frames}", flush=True)
    w32 = fp32().double().cpu()
    res["max_over_rms_native_vs_torch_fp32"] = R.rel_err(model(mel), w32)
    res["max_over_rms_autocast_vs_torch_fp32"] = R.rel_err(autocast().float(), w32)
    res["native_over_torch_fp32_min"] = res["native_ms_per_call"]["min"] / res["torch_fp32_ms_per_call"]["min"]
    res["native_over_torch_fp16_autocast_min"] = res["native_ms_per_call"]["min"] / res["torch_fp16_autocast_ms_per_call"]["min"]
    res["residual_convolutions_per_stage"] = []
    L = frames
    for i, u in enumerate(cfg["upsample_rates"]):
        L *= u
        fused, C = stage_convs(torch, model, i, B, L, True)
        unfused, _ = stage_convs(torch, model, i, B, L, False)
        arms = {"fused": fused, "unfused": unfused}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        t = windows(torch, arms, calls, REPS)
        res["residual_convolutions_per_stage"].append(dict(stage=i, channels=C, positions=L, fused_ms=summary(t["fused"], calls),
                                                           unfused_ms=summary(t["unfused"], calls),
                                                           fused_over_unfused_min=min(t["fused"]) / min(t["unfused"])))
        print(f"timed stage {i} ({C} channels, {L} positions): fused / unfused {min(t['fused']) / min(t['unfused']):.3f}", flush=True)
    return res


def profile(name, B, frames, fuse="default"):
    torch, R, cfg, _, model = setup(name)
    if fuse != "default":
        model.fuse_act_max_channels = {"everywhere": None, "nowhere": 0}[fuse]
    mel = R.mels(B, cfg["n_mels"], frames, 1).to("cuda")
    for _ in range(WARM + 3):
        model(mel)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bigvgan_times.json")
    results = {"note": f"ms per BigVGANGenerator call, random weights; device events around {REPS} alternating windows of back-to-back calls "
                       "per arm in one process (host side of the call included), one MI355X; torch_* = the same network from "
                       "torch.nn.functional on the same device (tools/bigvgan_times.py: torch_generator), in fp32 and under fp16 autocast; "
                       "native_fused_everywhere / native_fused_nowhere = the native path with Activation1d fused into every residual "
                       "convolution's staging / into none; residual_convolutions_per_stage = one stage's residual convolutions alone; "
                       "spread = (max - min) / min over the windows; produced by tools/bigvgan_times.py",
               "configs": {}}
    for name in ("BASE", "WIDE"):
        torch, R, cfg, sd, model = setup(name)
        ref = torch_generator(R, sd, cfg, "cuda")
        entry = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, "shapes": []}
        results["configs"][name] = entry
        for B, frames, calls in SHAPES:
            entry["shapes"].append(measure(torch, R, cfg, model, ref, B, frames, calls))
            with open(out, "w") as fh:  # after every shape: a later one that runs out of time loses nothing
                json.dump(results, fh, indent=1)
                fh.write("\n")
        del model, ref
        torch.cuda.empty_cache()
    print(json.dumps(results, indent=1))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:6])
    else:
        sys.exit(main())
