"""SEANetEncoder: the native launch sequence (csrc/seanet.hip + one GEMM) beside what a user would write without it -- the same
network from torch.nn.functional (F.pad, F.conv1d, F.elu) and nn.LSTM on the same device, in fp32 and under fp16 autocast.
EnCodec's 24 kHz widths (32 filters, ratios 8 5 4 2, 2-layer LSTM of 512, dimension 128), random weights.  One MI355X.

    python tools/seanet_times.py [OUT.json]            (default: profiles/seanet_times.json)
    python tools/seanet_times.py --profile B SAMPLES    (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

The parent runs one child process per shape under `timeout -k 10 <seconds>`, then one for the train step (dim 512, depth 12: a step
from 8 x 163 840-sample waves through EncodecVocoCodec(encoder=SEANetEncoder) beside the same step from precomputed latents); a
child that fails is reported and not run again, and nothing is started after it.  In a child the paths run in one process,
alternating, after warm-up, device events around windows of back-to-back calls (the host side of a call included); the minimum of
the windows is the figure for the encoder, the median of the steps for the train step."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 163840), (1, 24000)]
CALLS, REPS, WARM = 10, 5, 3
TRAIN_STEPS = 9


def torch_seanet(S, sd, cfg, dev):
    """the encoder from torch's own operators on `dev`: weight norm folded once, SConv1d's padding from tests/seanet_ref.py"""
    import torch
    import torch.nn.functional as F

    w, b, lstm = {}, {}, None
    for e in S.layout(cfg):
        i, kind = e[0], e[1]
        names = [f"model.{i}"] if kind == "conv" else [f"model.{i}.block.1", f"model.{i}.block.3", f"model.{i}.shortcut"] if kind == "res" else []
        for n in names:
            w[n], b[n] = S.fold(sd, n, torch.float32).to(dev), sd[f"{n}.conv.conv.bias"].to(dev)
        if kind == "lstm":
            lstm = torch.nn.LSTM(e[2], e[2], e[3])
            lstm.load_state_dict({k.split(".lstm.")[1]: v for k, v in sd.items() if k.startswith(f"model.{i}.lstm.")})
            lstm = lstm.to(dev).eval()

    def fwd(wave):
        x, act = wave[:, None], False
        for e in S.layout(cfg):
            i, kind = e[0], e[1]
            if kind == "elu":
                act = True
            elif kind == "conv":
                n = f"model.{i}"
                x = S.sconv(F.elu(x) if act else x, w[n], b[n], stride=e[5])
                act = False
            elif kind == "res":
                p = f"model.{i}"
                h = S.sconv(F.elu(x), w[p + ".block.1"], b[p + ".block.1"], dilation=e[5])
                x = S.sconv(x, w[p + ".shortcut"], b[p + ".shortcut"]) + S.sconv(F.elu(h), w[p + ".block.3"], b[p + ".block.3"])
            else:
                t = x.permute(2, 0, 1)
                x = (lstm(t)[0] + t).permute(1, 2, 0)
        return x.transpose(1, 2)

    return fwd


def setup(B, T):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seanet_ref as S
    import voicebox_pytorch_amd as vbx

    cfg = S.config()
    sd = S.random_state(cfg, 0)
    model = vbx.SEANetEncoder()
    model.load_state_dict(sd)
    model = model.to("cuda").eval()
    x = (0.3 * torch.randn(B, T, generator=torch.Generator().manual_seed(1))).to("cuda")
    return torch, S, cfg, sd, model, x


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


def child(B, T):
    torch, S, cfg, sd, model, x = setup(B, T)
    ref = torch_seanet(S, sd, cfg, "cuda")

    def fp32():
        with torch.inference_mode():
            return ref(x)

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return ref(x)

    paths = {"native": lambda: model(x), "torch_fp32": fp32, "torch_fp16_autocast": autocast}
    res = {"B": B, "samples": T, "frames": model.frames(T), **{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for k, v in windows(torch, paths, CALLS, REPS).items():
        res[k + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=CALLS, windows=REPS)
    w32 = fp32().double()
    res["max_over_rms_native_vs_torch_fp32"] = S.rel_err(model(x), w32.cpu())
    res["max_over_rms_autocast_vs_torch_fp32"] = S.rel_err(autocast(), w32.cpu())
    res["native_over_torch_fp32_min"] = res["native_ms_per_call"]["min"] / res["torch_fp32_ms_per_call"]["min"]
    res["native_over_torch_fp16_autocast_min"] = res["native_ms_per_call"]["min"] / res["torch_fp16_autocast_ms_per_call"]["min"]
    res["launches_per_call"] = len(model.packed_ops()) + (model.frames(T) + model.lstm - 1 if model.lstm else 0)  # the LSTM: a GEMM and its steps
    print("RESULT " + json.dumps(res))


def train_child(B, T):
    torch, S, cfg, sd, enc, wave = setup(B, T)
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep

    rvq = vbx.ResidualVQ(dim=128, codebook_size=1024, num_quantizers=8)
    rvq.load_state_dict({"codebooks": 0.5 ** torch.arange(8.0)[:, None, None] * torch.randn(8, 1024, 128, generator=torch.Generator().manual_seed(2))})
    voc = vbx.VocosDecoder(input_channels=128, dim=64, intermediate_dim=192, num_layers=1, n_fft=256, hop_length=64)  # not called in training
    codec = vbx.EncodecVocoCodec(rvq=rvq, vocoder=voc, encoder=enc, downsample_factor=enc.hop_length).to("cuda").eval()
    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=512, num_cond_tokens=500, depth=12, dim_head=64, heads=8, audio_enc_dec=codec, condition_on_text=False).to("cuda")
    ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb), lr=3e-4, max_grad_norm=0.5)
    latents = codec.encode(wave)
    paths = {"step_from_waves": lambda: ts.step(wave), "step_from_latents": lambda: ts.step(latents)}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    res = {"B": B, "samples": T, "frames": latents.shape[1], "dim": 512, "depth": 12}
    for k, v in windows(torch, paths, 1, TRAIN_STEPS).items():
        res[k + "_ms"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), steps=TRAIN_STEPS)
    res["encode_share_of_step_median"] = 1.0 - res["step_from_latents_ms"]["median"] / res["step_from_waves_ms"]["median"]
    print("RESULT " + json.dumps(res))


def profile(B, T):
    torch, _, _, _, model, x = setup(B, T)
    for _ in range(WARM + CALLS):
        model(x)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "seanet_times.json")
    results = {"note": f"ms per SEANetEncoder call at EnCodec's 24 kHz widths, random weights; device events around {REPS} alternating "
                       f"windows of {CALLS} back-to-back calls per path in one process (host side of the call included), one MI355X; torch_* "
                       "= the same network from torch.nn.functional + nn.LSTM on the same device (tools/seanet_times.py: torch_seanet), in "
                       "fp32 and under fp16 autocast; train_step: dim 512 / depth 12, medians of alternating single steps; produced by "
                       "tools/seanet_times.py", "shapes": []}
    jobs = [("--child", B, T, "shapes") for B, T in SHAPES] + [("--train-child", SHAPES[0][0], SHAPES[0][1], "train_step")]
    failed = False
    for mode, B, T, key in jobs:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), mode, str(B), str(T)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        ok = p.returncode == 0 and line
        entry = json.loads(line[0][7:]) if ok else {"B": B, "samples": T, "failed_rc": p.returncode, "stderr_tail": p.stderr[-600:]}
        if key == "shapes":
            results["shapes"].append(entry)
        else:
            results[key] = entry
        if not ok:
            failed = True
            break  # nothing more is started on the device after a failure
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 1 if failed else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--train-child":
        train_child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
