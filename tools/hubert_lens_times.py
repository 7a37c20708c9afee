"""Times of HubertWithKmeans(wave, lens=) and of the text-conditioned train step from ragged waves on one MI355X:
    python tools/hubert_lens_times.py [OUT.json] [--arms plain,full,ragged,step] [--tag NAME] [--tree DIR]
                                                        (default: profiles/hubert_lens_times.json, all arms, tag "branch", this tree)

    plain   tok(wave), BASE widths, layer 9, 8 x 160 000 samples, lens=None: the old launches.  `--arms plain --tag parent --tree DIR`
            runs the same call on a checkout of the parent commit (a tree without lens=); an existing OUT.json is updated under the
            --tag key, not replaced.  The difference must lie inside the window spread: lens=None launches what it launched.
    full    the same call with lens given and every row full, beside lens=None (what the *_lens kernels cost when they mask nothing)
    ragged  lengths spread over 40 .. 100 % of 160 000 samples, beside the same batch without lengths
    step    the dim-512 / depth-12 text-conditioned LogMelCodec train step from those waves (24 kHz) with wav2vec=tok: step(waves)
            and step(waves, wave_lens=)

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
B, T = 8, 160000
MODEL = dict(dim=512, depth=12, heads=16, dim_head=64)
LENS = [round(T * (0.4 + 0.6 * i / (B - 1))) for i in range(B)]  # 40 .. 100 %
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


def tokenizer():
    torch.manual_seed(0)
    return vbx.HubertWithKmeans(output_layer=9, codebook_size=500).to(dev)  # BASE widths, random weights: the times do not depend on them


def main():
    args = ARGS
    chosen, tag = (take(args, "--arms") or "plain,full,ragged,step").split(","), take(args, "--tag") or "branch"
    out = args[0] if args else os.path.join(HERE, "profiles", "hubert_lens_times.json")
    res = {}
    wave = 0.3 * torch.randn(B, T, device=dev)
    unit = "ms per call, min of %d windows of 10 back-to-back calls, host side included" % WINDOWS
    if {"plain", "full", "ragged"} & set(chosen):
        tok = tokenizer()
        arms = {"lens_none": lambda: tok(wave)}
        if "full" in chosen:
            full = torch.full((B,), T, dtype=torch.int32, device=dev)
            arms["full_lens"] = lambda: tok(wave, lens=full)
        if "ragged" in chosen:
            rag = torch.tensor(LENS, dtype=torch.int32, device=dev)  # no host read in the call
            arms["ragged_lens"] = lambda: tok(wave, lens=rag)
        row = measure(arms, 10)
        for n in ("full_lens", "ragged_lens"):
            if n in row:
                row[n]["ratio_to_lens_none"] = round(row[n]["ms"] / row["lens_none"]["ms"], 4)
        res["tokens"] = dict(unit=unit, shape=dict(B=B, samples=T, widths="BASE", output_layer=9, lens=LENS), arms=row)
    if "step" in chosen:
        from voicebox_pytorch_amd.dp import TrainStep

        torch.manual_seed(0)
        codec = vbx.LogMelCodec().to(dev)
        vb = vbx.VoiceBox(depth=MODEL["depth"], dim=MODEL["dim"], dim_head=64, heads=MODEL["heads"], audio_enc_dec=codec,
                          condition_on_text=True, num_cond_tokens=500).to(dev)
        ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb, wav2vec=tokenizer()), lr=1e-5, max_grad_norm=0.5)
        wl = torch.tensor(LENS, dtype=torch.int32, device=dev)
        arms = {"waves": lambda: ts.step(wave), "waves_wave_lens": lambda: ts.step(wave, wave_lens=wl)}
        row = measure(arms, 10)
        row["waves_wave_lens"]["ratio_to_waves"] = round(row["waves_wave_lens"]["ms"] / row["waves"]["ms"], 4)
        res["train_step"] = dict(unit="ms per train step, min of %d windows of 10 back-to-back steps, host side included" % WINDOWS,
                                 shape=dict(MODEL, B=B, samples=T, rate=codec.sampling_rate, codec="LogMelCodec", wav2vec="HubertWithKmeans BASE, layer 9",
                                            lens=LENS), arms=row)
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
