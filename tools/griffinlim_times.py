"""Griffin-Lim decode: the native loop (csrc/griffinlim.hip) beside what a user would write without it -- the same loop from
torch.stft / torch.istft on the same device in fp32 (tests/griffinlim_ref.py with device tensors).  One MI355X.

    python tools/griffinlim_times.py [OUT.json]        (default: profiles/griffinlim_times.json)

The parent runs one child process per shape under `timeout -k 10 <seconds>`; a child that fails is reported and not run again, and
nothing is started after it.  In a child both paths run in one process, alternating, after warm-up, device events around windows of
>= 20 calls each.  Bytes per iteration are computed from the shapes (what each launch must read and write once), not measured."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1025), (1, 301)]
CFG = dict(n_fft=1024, win_length=640, hop_length=160)
N_ITER, CALLS, REPS, WARM = 32, 20, 5, 3
HBM_PEAK, COPY_RATE = 8.0e12, 6.3e12  # bytes / s: HBM peak and the achievable copy rate of an MI355X


def child(B, frames):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import griffinlim_ref as gl
    import voicebox_pytorch_amd as vbx

    dev = "cuda"
    torch.manual_seed(0)
    nb = CFG["n_fft"] // 2 + 1
    mag = torch.rand(B, nb, frames, device=dev) * (torch.rand(B, nb, frames, device=dev) > 0.38)
    phase = (2 * torch.rand(B, nb, frames, device=dev) - 1) * torch.pi
    native = lambda: vbx.griffin_lim(mag, phase=phase, n_iter=N_ITER, **CFG)
    res = {"B": B, "frames": frames, "samples": (frames - 1) * CFG["hop_length"], "n_iter": N_ITER, **CFG}
    try:
        gl.griffin_lim(mag, phase, n_iter=1, dtype=torch.float32, **CFG)
        torch.cuda.synchronize()
        incumbent = lambda: gl.griffin_lim(mag, phase, n_iter=N_ITER, dtype=torch.float32, **CFG)
    except Exception as e:  # no device FFT in this torch build: recorded, the native time stands alone
        incumbent, res["torch_loop_unavailable"] = None, f"{type(e).__name__}: {e}"[:300]
    paths = {"native": native} if incumbent is None else {"native": native, "torch_loop": incumbent}
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
    if incumbent is not None:
        w_n, w_t = native().double(), incumbent().double()
        res["rel_l2_native_vs_torch_loop"] = float((w_n - w_t).norm() / w_t.norm())
        res["native_over_torch_loop_median"] = res["native_ms_per_call"]["median"] / res["torch_loop_ms_per_call"]["median"]
    # per iteration: synthesis reads two spectra (8 B / bin) and the magnitude, writes the frame buffer; analysis reads the frame
    # buffer and the reciprocal envelope once and writes one spectrum
    spec, fbuf = B * frames * nb * 8, B * frames * CFG["win_length"] * 4
    per_iter = (2 * spec + spec // 2 + fbuf) + (fbuf + (frames - 1) * CFG["hop_length"] * 4 + spec)
    t_iter = res["native_ms_per_call"]["median"] * 1e-3 / (N_ITER + 1)
    res.update(launches_per_iteration=2, launches_per_call=2 * N_ITER + 2, bytes_per_iteration=per_iter,
               native_us_per_iteration=t_iter * 1e6, implied_bytes_per_s=per_iter / t_iter,
               fraction_of_hbm_peak_8_0e12=per_iter / t_iter / HBM_PEAK, fraction_of_copy_rate_6_3e12=per_iter / t_iter / COPY_RATE)
    print("RESULT " + json.dumps(res))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "griffinlim_times.json")
    results = {"note": "ms per griffin_lim call (32 iterations; table look-ups and the initial phasors included), device events around "
                       f"{REPS} alternating windows of {CALLS} back-to-back calls per path in one process, one MI355X; torch_loop = "
                       "tests/griffinlim_ref.py (torch.stft / torch.istft) on the same device in fp32; bytes per iteration computed "
                       "from shapes; produced by tools/griffinlim_times.py", "shapes": []}
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
    else:
        sys.exit(main())
