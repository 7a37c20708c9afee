"""Sample-rate conversion: the native kernel (csrc/resample.hip) beside what a user would write without it -- the same polyphase
arithmetic as one strided F.conv1d on the same device in fp32 over an explicitly padded wave (tests/resample_ref.py with the bank
already on the device) -- and the in-situ cost: a dim-512 / depth-12 LogMelCodec train step from 16 kHz waves beside the step from
24 kHz waves of the same frame count.  One MI355X.

    python tools/resample_times.py [OUT.json]        (default: profiles/resample_times.json)

The parent runs one child process per measurement under `timeout -k 10 <seconds>`; a child that fails is reported and not run again,
and nothing is started after it.  In a child both paths run in one process, alternating, after warm-up, device events around windows
of back-to-back calls.  Bytes are computed from the shapes (input read once, output written once), not measured."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 163840, 16000), (8, 301056, 44100), (8, 327680, 48000)]  # the last two give 8 x 163 840 samples at 24 kHz
NEW = 24000
CALLS, REPS, WARM = 50, 5, 5
HBM_PEAK = 8.0e12  # bytes / s


def _windows(paths, calls):
    import torch

    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(REPS):  # alternating windows
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=calls, windows=REPS) for k, v in times.items()}


def child_kernel(B, L, orig):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_ref as R
    import voicebox_pytorch_amd as vbx

    dev = "cuda"
    torch.manual_seed(0)
    x = torch.randn(B, L, device=dev)
    ro, rn = R.reduced(orig, NEW)
    h, width = R.bank(orig, NEW)
    hd = h.float()[:, None, :].to(dev)
    Lout = -(-rn * L // ro)

    def conv1d():
        y = F.conv1d(F.pad(x[:, None], (width, width + ro)), hd, stride=ro)
        return y.transpose(1, 2).reshape(B, -1)[:, :Lout]

    native = lambda: vbx.resample(x, orig, NEW)
    res = {"B": B, "L": L, "orig_freq": orig, "new_freq": NEW, "Lout": Lout, "phases": rn, "taps": h.shape[1],
           "nonzero_taps_fraction": float((h.float() != 0).double().mean())}
    try:
        conv1d()
        torch.cuda.synchronize()
        paths = {"native": native, "conv1d": conv1d}
    except Exception as e:  # no device convolution for this shape in this torch build: recorded, the native time stands alone
        paths, res["conv1d_unavailable"] = {"native": native}, f"{type(e).__name__}: {e}"[:300]
    for k, v in _windows(paths, CALLS).items():
        res[k + "_ms_per_call"] = v
    if "conv1d" in paths:
        a, b = native().double(), conv1d().double()
        res["max_abs_native_minus_conv1d"] = float((a - b).abs().max())
        res["native_over_conv1d_min"] = res["native_ms_per_call"]["min"] / res["conv1d_ms_per_call"]["min"]
        res["faster_than_conv1d"] = res["native_ms_per_call"]["min"] < res["conv1d_ms_per_call"]["min"]
    nbytes = 4 * B * (L + Lout)
    t = res["native_ms_per_call"]["min"] * 1e-3
    res.update(bytes_in_plus_out=nbytes, us_at_hbm_peak_8_0e12=nbytes / HBM_PEAK * 1e6, implied_bytes_per_s=nbytes / t,
               fraction_of_hbm_peak_8_0e12=nbytes / t / HBM_PEAK)
    print("RESULT " + json.dumps(res))


def child_step():
    import torch

    sys.path.insert(0, ROOT)
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep

    dev = "cuda"
    torch.manual_seed(0)
    vb = vbx.VoiceBox(audio_enc_dec=vbx.LogMelCodec(), dim=512, depth=12, heads=16, dim_head=64, num_cond_tokens=500,
                      condition_on_text=False).to(dev)
    ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb, resample_input=True), lr=1e-4, max_grad_norm=0.5)
    w16, w24 = torch.randn(8, 109120, device=dev), torch.randn(8, 163680, device=dev)  # both 1024 frames of 160 samples at 24 kHz
    paths = {"from_16k_waves": lambda: ts.step(w16, input_sampling_rate=16000), "from_24k_waves": lambda: ts.step(w24)}
    res = {"model": "dim 512, depth 12, LogMelCodec, 8 x 1024 frames", **{k + "_ms_per_step": v for k, v in _windows(paths, 10).items()}}
    res["in_situ_cost_ms_median"] = res["from_16k_waves_ms_per_step"]["median"] - res["from_24k_waves_ms_per_step"]["median"]
    print("RESULT " + json.dumps(res))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample_times.json")
    results = {"note": "ms per resample call (bank look-up and the output allocation included), device events around "
                       f"{REPS} alternating windows of {CALLS} back-to-back calls per path in one process, one MI355X; conv1d = the same "
                       "arithmetic as a strided F.conv1d in fp32 over an explicitly padded wave, bank already on the device; the bar is "
                       "the min of the windows; bytes computed from shapes; train_step: windows of 10 steps; produced by "
                       "tools/resample_times.py", "shapes": [], "train_step": None}
    jobs = [("shapes", ["--child", str(B), str(L), str(o)]) for B, L, o in SHAPES] + [("train_step", ["--child-step"])]
    ok = True
    for where, args in jobs:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__)] + args
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        r = json.loads(line[0][7:]) if p.returncode == 0 and line else {"args": args, "failed_rc": p.returncode, "stderr_tail": p.stderr[-600:]}
        if where == "shapes":
            results["shapes"].append(r)
        else:
            results["train_step"] = r
        if "failed_rc" in r:
            ok = False
            break  # nothing more is started on the device after a failure
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child_kernel(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-step":
        child_step()
    else:
        sys.exit(main())
