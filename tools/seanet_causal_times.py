"""CausalSEANetEncoder / CausalSEANetDecoder beside the non-causal SEANetEncoder / SEANetDecoder of the same tree: the same
products on the same tiles, only the padding side and the trim differ, so they should cost the same -- this measures it.
EnCodec's 24 kHz widths (32 filters, ratios 8 5 4 2, 2-layer LSTM of 512, dimension 128), random weights.  One MI355X.

    python tools/seanet_causal_times.py [OUT.json]           (default: profiles/seanet_causal_times.json)

One process: per shape the two arms run alternating, after warm-up, device events around windows of back-to-back calls (the host
side of a call included); the minimum of the windows is the figure, max - min of the windows the spread."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 512), (1, 75)]  # (batch, frames): 8 x 163 840 samples, 1 x 24 000
CALLS, REPS, WARM = 10, 5, 3


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


def measure(torch, what, arms, x):
    paths = {k: (lambda m=m: m(x)) for k, m in arms.items()}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    res = {"network": what, "input": list(x.shape)}
    for k, v in windows(torch, paths, CALLS, REPS).items():
        res[k + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), spread=max(v) - min(v), calls=CALLS, windows=REPS)
    res["causal_over_non_causal_min"] = res["causal_ms_per_call"]["min"] / res["non_causal_ms_per_call"]["min"]
    res["causal_minus_non_causal_min_ms"] = res["causal_ms_per_call"]["min"] - res["non_causal_ms_per_call"]["min"]
    return res


def main():
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seanet_dec_ref as D
    import seanet_ref as S
    import voicebox_pytorch_amd as vbx

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "seanet_causal_times.json")

    def load(cls, sd):
        m = cls()
        m.load_state_dict(sd)
        return m.to("cuda").eval()

    esd, dsd = S.random_state(S.config(), 0), D.random_state(D.config(), 0)
    enc = {"non_causal": load(vbx.SEANetEncoder, esd), "causal": load(vbx.CausalSEANetEncoder, esd)}
    dec = {"non_causal": load(vbx.SEANetDecoder, dsd), "causal": load(vbx.CausalSEANetDecoder, dsd)}
    g = torch.Generator().manual_seed(1)
    shapes = []
    for B, frames in SHAPES:
        shapes.append(measure(torch, "encoder", enc, (0.3 * torch.randn(B, frames * 320, generator=g)).to("cuda")))
        shapes.append(measure(torch, "decoder", dec, (3.0 * torch.randn(B, 128, frames, generator=g)).to("cuda")))
    results = {"note": f"ms per call at EnCodec's 24 kHz widths, random weights, the same weights in both arms; device events around {REPS} "
                       f"alternating windows of {CALLS} back-to-back calls per arm in one process (host side of the call included), one "
                       "MI355X; causal = CausalSEANetEncoder / CausalSEANetDecoder, non_causal = SEANetEncoder / SEANetDecoder of the "
                       "same tree; spread = max - min over the windows; produced by tools/seanet_causal_times.py",
               "shapes": shapes}
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
