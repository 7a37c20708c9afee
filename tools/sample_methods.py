"""Times ConditionalFlowMatcherWrapper.sample for each ODE method at the benchmark shape (8 x 1024 frames, dim 512, depth 12, heads 16,
hipGraph), one process, the same call: midpoint at 64 intervals is the yardstick; euler and rk4 on the same grid; dopri5 at the default
tolerances on the benchmark's seeded weights (bench.py build_model) and on the well-conditioned config-5 weights
(restate.init_state_dict(seed=4), q / k norm gammas x 0.25 -- tests/test_model_gpu.py test_cfg5_depth12_64_interval_sample_vs_cpu_reference).
Prints one line per run: ms (median of --reps), NFE, ms per NFE, accepted / rejected; --out FILE also writes them as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--intervals", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import voicebox_pytorch_amd as vbx
    from oracle import restate

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)  # bench.py build_model
    vb = vbx.VoiceBox(dim=512, num_cond_tokens=500, depth=12, dim_head=64, heads=16, condition_on_text=False)
    with torch.no_grad():
        for name, p in vb.named_parameters():
            if ".to_gamma.weight" in name or ".to_beta." in name:
                p.normal_(0.0, 0.02)
    vb = vb.to(dev)
    torch.manual_seed(1234)
    x = torch.randn(args.batch, args.frames, 512, device=dev)
    state_wc = restate.init_state_dict(restate.Cfg(dim=512, depth=12, heads=16, dim_head=64), seed=4)
    for k in state_wc:
        if k.endswith("q_norm.gamma") or k.endswith("k_norm.gamma"):
            state_wc[k] = state_wc[k] * 0.25
    rows = []

    def run(label, method, weights="bench"):
        w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=method)
        steps = args.intervals + 1
        w.sample(cond=x, steps=steps)  # capture + warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w.sample(cond=x, steps=steps)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(ts)
        st = w.last_sample_stats
        r = dict(label=label, method=method, weights=weights, ms=round(ms, 2), runs_ms=[round(t, 2) for t in ts], nfe=st["nfe"],
                 ms_per_nfe=round(ms / st["nfe"], 4), accepted=st["accepted"], rejected=st["rejected"])
        rows.append(r)
        print(json.dumps(r), flush=True)
        del w
        torch.cuda.empty_cache()

    run("midpoint (yardstick)", "midpoint")
    run("euler", "euler")
    run("rk4", "rk4")
    run("dopri5", "dopri5")
    run("midpoint (yardstick, again)", "midpoint")
    missing = vb.load_state_dict(state_wc, strict=False)
    assert not missing.unexpected_keys
    run("dopri5 well-conditioned", "dopri5", weights="cfg5_wc")
    run("midpoint well-conditioned", "midpoint", weights="cfg5_wc")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(shape=dict(batch=args.batch, frames=args.frames, dim=512, depth=12, heads=16), intervals=args.intervals,
                           device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
