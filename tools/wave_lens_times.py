"""Times of ragged waves (lens= of the codec encoders, wave_lens= of the train step) on one MI355X:
    python tools/wave_lens_times.py [OUT.json] [--arms enc,enc_full,step] [--tag NAME] [--tree DIR]
                                                        (default: profiles/wave_lens_times.json, all arms, tag "branch", this tree)

    enc       LogMelCodec.encode(wave) and SEANetEncoder(wave) (24 kHz widths) at 8 x 163 840 samples, lens=None: the old entry points.
              `--arms enc --tag parent --tree DIR` runs the same two calls on a checkout of the parent commit (a tree without lens=);
              an existing OUT.json is updated under the --tag key, not replaced, so the parent's and the branch's figures land in one
              file.  The difference must lie inside the window spread: the old entry points launch the code they launched.
    enc_full  the same two calls with lens given and every row full (report only: what the *_lens instantiations cost when they mask
              nothing)
    step      the dim-512 / depth-12 LogMelCodec train step from 8 waves whose lengths give 410 .. 1024 frames: step(wave) (padding
              encoded and trained on as audio), step(wave, wave_lens=), and beside them the latent-side steps they become,
              step(latents) and step(latents, lens=frames) (report only)

Arms alternate in one process, window by window.  A window is CALLS back-to-back calls between two host synchronisations, wall clock,
host side included; the figure is the minimum of WINDOWS windows per call, every window is kept and max - min of an arm's windows
stands beside it."""
import json
import os
import sys
import time


def take(args, flag):
    if flag not in args:
        return None
    i = args.index(flag)
    v = args[i + 1]
    del args[i:i + 2]
    return v


ARGS = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(take(ARGS, "--tree") or HERE)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import voicebox_pytorch_amd as vbx  # noqa: E402

dev = "cuda"
B, T = 8, 163840
MODEL = dict(dim=512, depth=12, heads=16, dim_head=64)
FRAMES = [round(410 + i * (1024 - 410) / (B - 1)) for i in range(B)]  # the lengths of profiles/train_lens_times.json
WINDOWS = 5


def window(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def measure(arms, calls, warm=3):
    for fn in arms.values():
        for _ in range(warm):
            fn()
    wins = {n: [] for n in arms}
    for _ in range(WINDOWS):
        for n, fn in arms.items():  # the arms alternate
            wins[n].append(window(fn, calls))
    return {n: {"ms": round(min(w), 4), "windows": [round(x, 4) for x in w], "spread": round(max(w) - min(w), 4)} for n, w in wins.items()}


def encoders():
    torch.manual_seed(0)
    return vbx.LogMelCodec().to(dev), vbx.SEANetEncoder().to(dev).eval()


def main():
    args = ARGS
    chosen, tag = (take(args, "--arms") or "enc,enc_full,step").split(","), take(args, "--tag") or "branch"
    out = args[0] if args else os.path.join(HERE, "profiles", "wave_lens_times.json")
    res = {}
    wave = 0.3 * torch.randn(B, T, device=dev)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    if "enc" in chosen or "enc_full" in chosen:
        mel, enc = encoders()
        arms = {}
        if "enc" in chosen:
            arms.update(logmel=lambda: mel.encode(wave), seanet=lambda: enc(wave))
        if "enc_full" in chosen:
            arms.update(logmel_full_lens=lambda: mel.encode(wave, lens=full), seanet_full_lens=lambda: enc(wave, lens=full))
        res["encode"] = dict(unit="ms per call, min of %d windows of 10 back-to-back calls, host side included" % WINDOWS,
                             shape=dict(B=B, samples=T), arms=measure(arms, 10))
    if "step" in chosen:
        from voicebox_pytorch_amd.dp import TrainStep

        torch.manual_seed(0)
        codec = vbx.LogMelCodec().to(dev)
        vb = vbx.VoiceBox(depth=MODEL["depth"], dim=MODEL["dim"], dim_head=64, heads=MODEL["heads"], audio_enc_dec=codec,
                          condition_on_text=False).to(dev)
        ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb), lr=1e-5, max_grad_norm=0.5)
        Ts = (max(FRAMES) - 1) * codec.hop_length
        waves = 0.3 * torch.randn(B, Ts, device=dev)
        wl = torch.tensor([(f - 1) * codec.hop_length for f in FRAMES], dtype=torch.int32, device=dev)  # no host read in the step
        fl = codec.frame_lens(wl)
        assert fl.tolist() == FRAMES
        lat = codec.encode(waves, lens=wl)
        arms = {"waves": lambda: ts.step(waves), "waves_wave_lens": lambda: ts.step(waves, wave_lens=wl),
                "latents": lambda: ts.step(lat), "latents_lens": lambda: ts.step(lat, lens=fl)}
        row = measure(arms, 10)
        row["waves_wave_lens"]["ratio_to_waves"] = round(row["waves_wave_lens"]["ms"] / row["waves"]["ms"], 4)
        row["latents_lens"]["ratio_to_latents"] = round(row["latents_lens"]["ms"] / row["latents"]["ms"], 4)
        res["train_step"] = dict(unit="ms per train step, min of %d windows of 10 back-to-back steps, host side included" % WINDOWS,
                                 shape=dict(MODEL, B=B, samples=Ts, codec="LogMelCodec", frames=FRAMES), arms=row)
    print(json.dumps({tag: res}), flush=True)
    doc = {}
    if os.path.exists(out):
        with open(out) as fh:
            doc = json.load(fh)
    doc[tag] = res
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
