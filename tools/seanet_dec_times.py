"""SEANetDecoder: the native launch sequence (csrc/seanet.hip + one GEMM) beside what a user would write without it -- the same
network from torch.nn.functional (F.conv_transpose1d, F.conv1d, F.elu) and nn.LSTM on the same device, in fp32 and under fp16
autocast.  EnCodec's 24 kHz widths (32 filters, ratios 8 5 4 2, 2-layer LSTM of 512, dimension 128), random weights.  One MI355X.

    python tools/seanet_dec_times.py [OUT.json]           (default: profiles/seanet_dec_times.json)
    python tools/seanet_dec_times.py --profile B FRAMES    (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

One process: per shape the three paths run alternating, after warm-up, device events around windows of back-to-back calls (the host
side of a call included); the minimum of the windows is the figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 512), (1, 75)]
CALLS, REPS, WARM = 10, 5, 3


def torch_seanet_decoder(D, S, sd, cfg, dev):
    """the decoder from torch's own operators on `dev`: weight norm folded once, the padding and the trim from the restatement"""
    import torch
    import torch.nn.functional as F

    w, b, lstm = {}, {}, None
    for e in D.layout(cfg):
        i, kind = e[0], e[1]
        names = [f"model.{i}"] if kind == "conv" else [f"model.{i}.block.1", f"model.{i}.block.3", f"model.{i}.shortcut"] if kind == "res" else []
        for n in names:
            w[n], b[n] = S.fold(sd, n, torch.float32).to(dev), sd[f"{n}.conv.conv.bias"].to(dev)
        if kind == "convtr":
            w[f"model.{i}"], b[f"model.{i}"] = D.fold_tr(sd, f"model.{i}", torch.float32).to(dev), sd[f"model.{i}.convtr.convtr.bias"].to(dev)
        if kind == "lstm":
            lstm = torch.nn.LSTM(e[2], e[2], e[3])
            lstm.load_state_dict({k.split(".lstm.")[1]: v for k, v in sd.items() if k.startswith(f"model.{i}.lstm.")})
            lstm = lstm.to(dev).eval()

    def fwd(z):
        x, act = z, False
        for e in D.layout(cfg):
            i, kind = e[0], e[1]
            n = f"model.{i}"
            if kind == "elu":
                act = True
            elif kind == "conv":
                x = S.sconv(F.elu(x) if act else x, w[n], b[n])
                act = False
            elif kind == "convtr":
                x = D.sconvtr(F.elu(x), w[n], b[n], e[5])
                act = False
            elif kind == "res":
                h = S.sconv(F.elu(x), w[n + ".block.1"], b[n + ".block.1"], dilation=e[5])
                x = S.sconv(x, w[n + ".shortcut"], b[n + ".shortcut"]) + S.sconv(F.elu(h), w[n + ".block.3"], b[n + ".block.3"])
            else:
                t = x.permute(2, 0, 1)
                x = (lstm(t)[0] + t).permute(1, 2, 0)
        return x[:, 0]

    return fwd


def setup():
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seanet_dec_ref as D
    import seanet_ref as S
    import voicebox_pytorch_amd as vbx

    cfg = D.config()
    sd = D.random_state(cfg, 0)
    model = vbx.SEANetDecoder()
    model.load_state_dict(sd)
    return torch, D, S, cfg, sd, model.to("cuda").eval()


def latents(torch, B, frames):
    return (3.0 * torch.randn(B, 128, frames, generator=torch.Generator().manual_seed(1))).to("cuda")


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


def measure(torch, D, cfg, model, ref, B, frames):
    z = latents(torch, B, frames)

    def fp32():
        with torch.inference_mode():
            return ref(z)

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return ref(z)

    paths = {"native": lambda: model(z), "torch_fp32": fp32, "torch_fp16_autocast": autocast}
    res = {"B": B, "frames": frames, "samples": frames * model.hop_length, **{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for k, v in windows(torch, paths, CALLS, REPS).items():
        res[k + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=CALLS, windows=REPS)
    w32 = fp32().double().cpu()
    res["max_over_rms_native_vs_torch_fp32"] = D.rel_err(model(z), w32)
    res["max_over_rms_autocast_vs_torch_fp32"] = D.rel_err(autocast().float(), w32)
    res["native_over_torch_fp32_min"] = res["native_ms_per_call"]["min"] / res["torch_fp32_ms_per_call"]["min"]
    res["native_over_torch_fp16_autocast_min"] = res["native_ms_per_call"]["min"] / res["torch_fp16_autocast_ms_per_call"]["min"]
    # the pack, every other entry of the launch list once, and for the LSTM a GEMM and its frames + layers - 1 steps
    res["launches_per_call"] = 1 + len(model.packed_ops()) + (frames + model.lstm - 1 if model.lstm else 0)
    return res


def profile(B, frames):
    torch, _, _, _, _, model = setup()
    z = latents(torch, B, frames)
    for _ in range(WARM + CALLS):
        model(z)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "seanet_dec_times.json")
    torch, D, S, cfg, sd, model = setup()
    ref = torch_seanet_decoder(D, S, sd, cfg, "cuda")
    results = {"note": f"ms per SEANetDecoder call at EnCodec's 24 kHz widths, random weights; device events around {REPS} alternating "
                       f"windows of {CALLS} back-to-back calls per path in one process (host side of the call included), one MI355X; "
                       "torch_* = the same network from torch.nn.functional + nn.LSTM on the same device (tools/seanet_dec_times.py: "
                       "torch_seanet_decoder), in fp32 and under fp16 autocast; produced by tools/seanet_dec_times.py",
               "shapes": [measure(torch, D, cfg, model, ref, B, frames) for B, frames in SHAPES]}
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
