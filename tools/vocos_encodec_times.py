"""VocosEncodecDecoder: the native launch sequence (csrc/vocos.hip + the GEMMs + vbx_istft_trim at n_fft 1280, padding="same") beside
what a user would write without it -- the same network from torch.nn.functional with Vocos's own "same" ISTFT (torch.fft.irfft +
F.fold) on the same device, in fp32 and under fp16 autocast.  Published vocos-encodec-24khz widths 128 / 384 / 1152 / 8 layers /
n_fft 1280 / hop 320 / 4 bandwidth ids, random weights.  One MI355X.

    python tools/vocos_encodec_times.py [OUT.json]        (default: profiles/vocos_encodec_times.json)
    python tools/vocos_encodec_times.py --profile B FRAMES     (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

The parent runs one child process per shape under `timeout -k 10 <seconds>`; a child that fails is reported and not run again, and
nothing is started after it.  In a child the paths run in one process, alternating, after warm-up, device events around windows of
back-to-back calls (the host side of a call included); the minimum of the windows is the figure."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 512), (1, 75)]
CFG = dict(input_channels=128, dim=384, intermediate_dim=1152, num_layers=8, n_fft=1280, hop_length=320, adanorm_num_embeddings=4)
BANDWIDTH_ID = 2
CALLS, REPS, WARM = 10, 5, 3


def torch_vocos_encodec(sd, cfg, dev):
    """the decoder from torch.nn.functional building blocks, AdaLayerNorm as layer_norm(x) * scale[id] + shift[id], ISTFT "same" as
    the published model writes it"""
    import torch
    import torch.nn.functional as F

    w = {k: v.to(dev) for k, v in sd.items()}
    dim, n_fft, hop, layers = cfg["dim"], cfg["n_fft"], cfg["hop_length"], cfg["num_layers"]
    pad = (n_fft - hop) // 2

    def fwd(x, i):
        ada = lambda t, name: F.layer_norm(t, (dim,), None, None, 1e-6) * w[name + ".scale.weight"][i] + w[name + ".shift.weight"][i]
        x = F.conv1d(x, w["backbone.embed.weight"], w["backbone.embed.bias"], padding=3)
        x = ada(x.transpose(1, 2), "backbone.norm").transpose(1, 2)
        for l in range(layers):
            p = f"backbone.convnext.{l}."
            h = F.conv1d(x, w[p + "dwconv.weight"], w[p + "dwconv.bias"], padding=3, groups=dim).transpose(1, 2)
            h = F.gelu(F.linear(ada(h, p + "norm"), w[p + "pwconv1.weight"], w[p + "pwconv1.bias"]))
            h = w[p + "gamma"] * F.linear(h, w[p + "pwconv2.weight"], w[p + "pwconv2.bias"])
            x = x + h.transpose(1, 2)
        o = F.layer_norm(x.transpose(1, 2), (dim,), w["backbone.final_layer_norm.weight"], w["backbone.final_layer_norm.bias"], 1e-6)
        o = F.linear(o, w["head.out.weight"], w["head.out.bias"]).float()
        m, p = o.transpose(1, 2).chunk(2, dim=1)
        spec = torch.clip(torch.exp(m), max=100.0) * (torch.cos(p) + 1j * torch.sin(p))
        T = spec.shape[2]
        window = w["head.istft.window"]
        ifft = torch.fft.irfft(spec, n_fft, dim=1, norm="backward") * window[None, :, None]
        size = (T - 1) * hop + n_fft
        y = F.fold(ifft, output_size=(1, size), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, pad:-pad]
        env = F.fold(window.square().expand(1, T, -1).transpose(1, 2), output_size=(1, size), kernel_size=(1, n_fft), stride=(1, hop))
        return y / env.squeeze()[pad:-pad]

    return fwd


def setup(B, frames):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vocos_ref as vr
    import vocos_same_ref as sr
    import voicebox_pytorch_amd as vbx

    sd = sr.random_state(CFG["input_channels"], CFG["dim"], CFG["intermediate_dim"], CFG["num_layers"], CFG["n_fft"], seed=0,
                         rows=CFG["adanorm_num_embeddings"])
    for i in range(CFG["num_layers"]):  # a stack of eight blocks at gamma ~ 1 / layers, as the published initialisation
        sd[f"backbone.convnext.{i}.gamma"] = sd[f"backbone.convnext.{i}.gamma"] / CFG["num_layers"]
    model = vbx.VocosEncodecDecoder(**CFG, bandwidth_id=BANDWIDTH_ID)
    model.load_state_dict(sd)
    model = model.to("cuda").eval()
    x = torch.randn(B, CFG["input_channels"], frames, generator=torch.Generator().manual_seed(1)).to("cuda")
    return torch, vr, sd, model, x


def child(B, frames):
    torch, vr, sd, model, x = setup(B, frames)
    ref = torch_vocos_encodec(sd, CFG, "cuda")

    def fp32():
        with torch.inference_mode():
            return ref(x, BANDWIDTH_ID)

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return ref(x, BANDWIDTH_ID)

    paths = {"native": lambda: model(x), "torch_fp32": fp32, "torch_fp16_autocast": autocast}
    try:
        fp32()
        torch.cuda.synchronize()
    except Exception as e:  # no device FFT in this torch build: recorded, the native time stands alone
        paths = {"native": paths["native"]}
        torch_unavailable = f"{type(e).__name__}: {e}"[:300]
    flop = 2.0 * B * frames * CFG["dim"] * (7 * CFG["input_channels"] + CFG["num_layers"] * 2 * CFG["intermediate_dim"] + CFG["n_fft"] + 2)
    res = {"B": B, "frames": frames, "samples": frames * CFG["hop_length"], "gemm_gflop": flop * 1e-9, "padding": "same",
           "bandwidth_id": BANDWIDTH_ID, **CFG}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(REPS):  # alternating windows
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / CALLS)
    for k, v in times.items():
        res[k + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=CALLS, windows=REPS)
    if len(paths) == 1:
        res["torch_unavailable"] = torch_unavailable
        print("RESULT " + json.dumps(res))
        return
    w32 = fp32().double()
    res["max_over_rms_native_vs_torch_fp32"] = vr.wave_err(model(x), w32)
    res["max_over_rms_autocast_vs_torch_fp32"] = vr.wave_err(autocast(), w32)
    res["native_over_torch_fp32_min"] = res["native_ms_per_call"]["min"] / res["torch_fp32_ms_per_call"]["min"]
    res["native_over_torch_fp16_autocast_min"] = res["native_ms_per_call"]["min"] / res["torch_fp16_autocast_ms_per_call"]["min"]
    res["native_gemm_tflops_at_min"] = flop / (res["native_ms_per_call"]["min"] * 1e-3) * 1e-12
    res["launches_per_call"] = 3 + 3 * CFG["num_layers"] + 5
    print("RESULT " + json.dumps(res))


def profile(B, frames):
    torch, _, _, model, x = setup(B, frames)
    for _ in range(WARM + CALLS):
        model(x)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocos_encodec_times.json")
    results = {"note": f"ms per VocosEncodecDecoder call at the published vocos-encodec-24khz widths, random weights; device events around "
                       f"{REPS} alternating windows of {CALLS} back-to-back calls per path in one process (host side of the call "
                       "included), one MI355X; torch_* = the same network from torch.nn.functional with torch.fft.irfft + F.fold on the "
                       "same device (tools/vocos_encodec_times.py: torch_vocos_encodec), in fp32 and under fp16 autocast; gemm_gflop "
                       "counts the GEMMs only; produced by tools/vocos_encodec_times.py", "shapes": []}
    for B, frames in SHAPES:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(B), str(frames)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results["shapes"].append({"B": B, "frames": frames, "failed_rc": p.returncode, "stderr_tail": p.stderr[-600:]})
            break  # nothing more is started on the device after a failure
        results["shapes"].append(json.loads(line[0][7:]))
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 0 if all("failed_rc" not in s for s in results["shapes"]) else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
