"""HiFiGANGenerator: the native launch sequence (csrc/hifigan.hip) beside what a user would write without it -- the same network from
torch.nn.functional (F.conv1d, F.conv_transpose1d, F.leaky_relu) on the same device, in fp32 and under fp16 autocast.  HiFi-GAN V1's
widths (80 mels, 512 channels, rates 8 8 2 2, kernels 3 7 11, dilations 1 3 5), random weights.  One MI355X.

    python tools/hifigan_times.py [OUT.json]            (default: profiles/hifigan_times.json)
    python tools/hifigan_times.py --profile B FRAMES     (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

One process: per shape the arms run alternating, after warm-up, device events around windows of back-to-back calls (the host side of
a call included); the minimum of the windows is the figure, their spread is recorded.  The native path runs twice more as the A/B
behind its dispatch rule: with the fused residual pair (vbx_hifigan_respair) at every width it serves, and without it; and per
narrow stage the residual blocks alone, fused against unfused."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024, 4), (1, 301, 10)]  # B, frames, calls per window
REPS, WARM = 5, 2


def torch_generator(H, sd, cfg, dev):
    """the generator from torch's own operators on `dev`, weight norm folded once"""
    import torch
    import torch.nn.functional as F

    w = {p: H.fold(sd, p, torch.float32).to(dev) for p, *_ in H.layout(cfg)}
    b = {p: sd[f"{p}.bias"].to(dev) for p, *_ in H.layout(cfg)}
    nk = len(cfg["resblock_kernel_sizes"])

    def conv(x, p, d=1):
        k = w[p].shape[-1]
        return F.conv1d(x, w[p], b[p], dilation=d, padding=(k - 1) * d // 2)

    def fwd(mel):
        x = conv(mel, "conv_pre")
        for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
            x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w[f"ups.{i}"], b[f"ups.{i}"], stride=u, padding=(k - u) // 2)
            xs = None
            for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
                rb, h = f"resblocks.{i * nk + j}", x
                for m, d in enumerate(ds):
                    t = conv(F.leaky_relu(h, 0.1), f"{rb}.convs1.{m}", d)
                    h = conv(F.leaky_relu(t, 0.1), f"{rb}.convs2.{m}") + h
                xs = h if xs is None else xs + h
            x = xs / nk
        return torch.tanh(conv(F.leaky_relu(x), "conv_post"))[:, 0]

    return fwd


def setup():
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hifigan_ref as H
    import voicebox_pytorch_amd as vbx

    cfg = H.V1
    sd = H.random_state(cfg, 0)
    model = vbx.HiFiGANGenerator(**cfg)
    model.load_state_dict(sd)
    return torch, H, cfg, sd, model.to("cuda").eval()


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
        model.fuse_max_channels = width
        try:
            return fn()
        finally:
            model.fuse_max_channels = type(model).FUSE_MAX_CHANNELS
    return run


def stage_blocks(torch, model, stage, B, L, fused):
    """the residual blocks of one stage alone on a random activation [B, L, C]: 9 pairs at V1, fused or as two launches each"""
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.hifigan import LRELU_SLOPE

    ops = model.packed_ops()["stages"][stage]
    C = ops["C"] // 2
    x = torch.randn(B, L, C, generator=torch.Generator().manual_seed(stage)).half().to("cuda")
    y = [torch.empty_like(x) for _ in range(3)]

    def run():
        st = _lib.current_stream()
        for block in ops["blocks"]:
            h, n = x, 0
            for c1, c2 in block:
                out = y[n % 2]
                if fused:
                    _lib.call("vbx_hifigan_respair", h, c1["w"], c1["b"], c2["w"], c2["b"], out, B, L, C, c1["k"], c1["dil"], LRELU_SLOPE, st)
                else:
                    _lib.call("vbx_hifigan_conv", h, c1["w"], c1["b"], None, y[2], B, L, C, C, c1["k"], c1["dil"], 1, LRELU_SLOPE, st)
                    _lib.call("vbx_hifigan_conv", y[2], c2["w"], c2["b"], h, out, B, L, C, C, c2["k"], 1, 1, LRELU_SLOPE, st)
                h, n = out, n + 1
    return run, C


def measure(torch, H, cfg, model, ref, B, frames, calls):
    mel = H.mels(B, cfg["n_mels"], frames, 1).to("cuda")

    def fp32():
        with torch.inference_mode():
            return ref(mel)

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return ref(mel)

    paths = {"native": lambda: model(mel), "torch_fp32": fp32, "torch_fp16_autocast": autocast,
             "native_fused_to_64": with_fuse(model, 64, lambda: model(mel)), "native_fused_to_32": with_fuse(model, 32, lambda: model(mel)),
             "native_unfused": with_fuse(model, 0, lambda: model(mel))}
    res = {"B": B, "frames": frames, "samples": frames * model.hop_length, "default_fuse_max_channels": model.fuse_max_channels,
           **{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}}
    for name, fn in paths.items():
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        print(f"warmed {name} at B {B} frames {frames}", flush=True)
    for k, v in windows(torch, paths, calls, REPS).items():
        res[k + "_ms_per_call"] = summary(v, calls)
    print(f"timed the whole network at B {B} frames {frames}", flush=True)
    w32 = fp32().double().cpu()
    res["max_over_rms_native_vs_torch_fp32"] = H.rel_err(model(mel), w32)
    res["max_over_rms_autocast_vs_torch_fp32"] = H.rel_err(autocast().float(), w32)
    res["native_over_torch_fp32_min"] = res["native_ms_per_call"]["min"] / res["torch_fp32_ms_per_call"]["min"]
    res["native_over_torch_fp16_autocast_min"] = res["native_ms_per_call"]["min"] / res["torch_fp16_autocast_ms_per_call"]["min"]
    res["residual_blocks_per_stage"] = []
    L = frames
    for i, u in enumerate(cfg["upsample_rates"]):
        L *= u
        if model.packed_ops()["stages"][i]["C"] // 2 > 64:
            continue
        fused, C = stage_blocks(torch, model, i, B, L, True)
        unfused, _ = stage_blocks(torch, model, i, B, L, False)
        arms = {"fused": fused, "unfused": unfused}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        t = windows(torch, arms, calls, REPS)
        res["residual_blocks_per_stage"].append(dict(stage=i, channels=C, positions=L, fused_ms=summary(t["fused"], calls),
                                                     unfused_ms=summary(t["unfused"], calls),
                                                     fused_over_unfused_min=min(t["fused"]) / min(t["unfused"])))
    return res


def profile(B, frames):
    torch, H, cfg, _, model = setup()
    mel = H.mels(B, cfg["n_mels"], frames, 1).to("cuda")
    for _ in range(WARM + 3):
        model(mel)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hifigan_times.json")
    torch, H, cfg, sd, model = setup()
    ref = torch_generator(H, sd, cfg, "cuda")
    results = {"note": f"ms per HiFiGANGenerator call at HiFi-GAN V1's widths, random weights; device events around {REPS} alternating windows "
                       "of back-to-back calls per arm in one process (host side of the call included), one MI355X; torch_* = the same "
                       "network from torch.nn.functional on the same device (tools/hifigan_times.py: torch_generator), in fp32 and under "
                       "fp16 autocast; native_fused_to_N / native_unfused = the native path with the fused residual pair at widths up to "
                       "N / nowhere; residual_blocks_per_stage = one stage's nine residual pairs alone; spread = (max - min) / min over "
                       "the windows; produced by tools/hifigan_times.py",
               "shapes": []}
    for B, frames, calls in SHAPES:
        results["shapes"].append(measure(torch, H, cfg, model, ref, B, frames, calls))
        with open(out, "w") as fh:  # after every shape: a later one that runs out of time loses nothing
            json.dump(results, fh, indent=1)
            fh.write("\n")
    print(json.dumps(results, indent=1))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
