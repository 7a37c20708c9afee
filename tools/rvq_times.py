"""EncodecVocoCodec: the native residual-VQ kernels (csrc/rvq.hip) beside the same arithmetic written with torch on the same device
in fp32 -- per stage: matmul, add |c|^2, argmin, gather, subtract; the gather-sum as Q indexed adds and a transpose.  Published
widths (dim 128, 1024 codewords, 8 quantizers), random codebooks, frames that lie near sums of codewords.  One MI355X.

    python tools/rvq_times.py [OUT.json]            (default: profiles/rvq_times.json)
    python tools/rvq_times.py --profile B FRAMES    (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

Three figures per shape: decode_to_codes (the search), codes_to_features (the gather-sum, channel-first), and the whole decode
(search + features + VocosDecoder; the torch arm of that one uses the torch search and gather in front of the SAME native vocoder, a
Vocos-EnCodec sized backbone: 128 -> 384 / 1152 x 8 layers, with an n_fft 1024 / hop 256 head because the inverse transform serves
powers of two).

The parent runs one child process per shape under `timeout -k 10 <seconds>`; a child that fails is reported and nothing is started
after it.  In a child both paths run in one process, alternating, after warm-up, device events around windows of back-to-back
calls (the host side of a call included); the minimum of the windows is the figure."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024), (1, 301)]
D, K, Q = 128, 1024, 8
VOC = dict(input_channels=128, dim=384, intermediate_dim=1152, num_layers=8, n_fft=1024, hop_length=256)
CALLS, REPS, WARM = 10, 5, 3


def torch_search(cb, norms):
    """decode_to_codes with torch: latents [B, N, D] -> codes [B, Q, N]"""
    import torch

    def fwd(z):
        B, N, _ = z.shape
        r = z.reshape(B * N, -1)
        codes = []
        for q in range(cb.shape[0]):
            k = torch.argmin(norms[q][None, :] - 2.0 * (r @ cb[q].t()), dim=1)
            codes.append(k)
            r = r - cb[q][k]
        return torch.stack(codes, dim=0).reshape(len(codes), B, N).transpose(0, 1).contiguous()

    return fwd


def torch_features(cb):
    def fwd(codes):  # [B, Q, N] -> [B, D, N]
        acc = cb[0][codes[:, 0]]
        for q in range(1, codes.shape[1]):
            acc = acc + cb[q][codes[:, q]]
        return acc.transpose(1, 2).contiguous()

    return fwd


def setup(B, frames):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rvq_ref as rr
    import vocos_ref as vr
    import voicebox_pytorch_amd as vbx

    x, cb = rr.random_case(B * frames, D, K, Q, seed=0)
    rvq = vbx.ResidualVQ(dim=D, codebook_size=K, num_quantizers=Q)
    rvq.load_state_dict({"codebooks": cb})
    voc = vbx.VocosDecoder(**VOC)
    sd = vr.random_state(VOC["input_channels"], VOC["dim"], VOC["intermediate_dim"], VOC["num_layers"], VOC["n_fft"], seed=0)
    for i in range(VOC["num_layers"]):
        sd[f"backbone.convnext.{i}.gamma"] = sd[f"backbone.convnext.{i}.gamma"] / VOC["num_layers"]
    voc.load_state_dict(sd)
    codec = vbx.EncodecVocoCodec(rvq=rvq, vocoder=voc, downsample_factor=VOC["hop_length"]).to("cuda").eval()
    return torch, rr, codec, x, cb


def child(B, frames):
    torch, rr, codec, x, cb = setup(B, frames)
    z = x.reshape(B, frames, D).to("cuda")
    cbd = codec.rvq.codebooks
    t_search, t_feat = torch_search(cbd, cbd.pow(2).sum(2)), torch_features(cbd)
    codes = codec.decode_to_codes(z)

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    paths = {
        "decode_to_codes": (lambda: codec.decode_to_codes(z), nograd(lambda: t_search(z))),
        "codes_to_features": (lambda: codec.codes_to_features(codes, check=False), nograd(lambda: t_feat(codes))),
        "decode": (lambda: codec.decode(z), nograd(lambda: codec.vocoder(t_feat(t_search(z))))),
    }
    res = {"B": B, "frames": frames, "dim": D, "codebook_size": K, "num_quantizers": Q, "vocoder": VOC,
           "search_gflop": 2.0 * B * frames * K * D * Q * 1e-9}
    for nat, ref in paths.values():
        for _ in range(WARM):
            nat()
            ref()
    torch.cuda.synchronize()
    times = {(k, arm): [] for k in paths for arm in ("native", "torch_fp32")}
    for _ in range(REPS):  # alternating windows
        for k, fns in paths.items():
            for arm, fn in zip(("native", "torch_fp32"), fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(CALLS):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[(k, arm)].append(a.elapsed_time(b) / CALLS)
    for k in paths:
        entry = {}
        for arm in ("native", "torch_fp32"):
            v = times[(k, arm)]
            entry[arm + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=CALLS, windows=REPS)
        entry["native_over_torch_fp32_min"] = entry["native_ms_per_call"]["min"] / entry["torch_fp32_ms_per_call"]["min"]
        res[k] = entry
    res["decode_to_codes"]["native_search_tflops_at_min"] = res["search_gflop"] / res["decode_to_codes"]["native_ms_per_call"]["min"]
    # results must not differ beyond what the contract allows: both searches against the fp64 checker, and against each other
    flat = lambda c: c.transpose(1, 2).reshape(B * frames, Q).cpu()
    tcodes = t_search(z)
    res["contract_native"] = rr.check_search(x, cb, flat(codes))
    res["contract_torch_fp32"] = rr.check_search(x, cb, flat(tcodes))
    res["frames_with_identical_codes"] = float((codes == tcodes).all(dim=1).float().mean())
    res["features_bit_equal"] = bool(torch.equal(codec.codes_to_features(codes), t_feat(codes)))
    print("RESULT " + json.dumps(res))


def profile(B, frames):
    torch, _, codec, x, _ = setup(B, frames)
    z = x.reshape(B, frames, D).to("cuda")
    for _ in range(WARM + CALLS):
        codec.decode(z)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rvq_times.json")
    results = {"note": f"ms per call at the published EnCodec widths (dim {D}, {K} codewords, {Q} quantizers), random codebooks; device "
                       f"events around {REPS} alternating windows of {CALLS} back-to-back calls per path in one process (host side of "
                       "the call included), one MI355X; torch_fp32 = the same arithmetic with torch on the same device "
                       "(tools/rvq_times.py: torch_search, torch_features); the two arms of `decode` share the native vocoder; "
                       "contract_* = tests/rvq_ref.py check_search of each arm's codes; produced by tools/rvq_times.py", "shapes": []}
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
