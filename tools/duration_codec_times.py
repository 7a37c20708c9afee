"""Times of DurationPredictor over codec latents (attach_codec) on one MI355X:
    python tools/duration_codec_times.py [OUT.json]        (default: profiles/duration_codec_times.json)

Three arms alternate in one process, window by window, over the same weights:
  fused   -- the predictor with the codec attached, fed the latents: proj_in, mask, drop, curtail_or_pad and the embedding gather in
             the one launch of vbx_pack_phoneme_latent (training: + the three launches that form d proj_in.weight / bias);
  linear  -- a codec-free predictor fed torch.nn.functional.linear(latents, proj_in.weight, proj_in.bias), which writes the
             [B, S, dim] projection to memory for vbx_pack_phoneme_input to read.  That path passes no gradient to cond, so this arm's
             backward does NOT compute d proj_in: in training it does less work than the fused arm;
  plain   -- the codec-free predictor fed a ready [B, S, dim] condition: what the parent commit could run, for context.
Per latent width and shape: eval forward, and forward + backward of the given-durations branch.  A window is 10 back-to-back calls
between two host synchronisations, wall clock, host side included; the figure is the minimum of five windows per call (the method
of tools/duration_train_times.py)."""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voicebox_pytorch_amd as vbx  # noqa: E402
from toy_codec import ToyCodec  # noqa: E402

dev = "cuda"
MODEL = dict(dim=512, depth=10, heads=8, dim_head=64, dim_phoneme_emb=512, num_phoneme_tokens=256)
LATENTS = (100, 128)
SHAPES = [(8, 200), (1, 60)]  # B, n (phonemes = latent frames)
CALLS, WINDOWS = 10, 5


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / CALLS * 1e3


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "duration_codec_times.json")
    torch.manual_seed(0)
    res = {"unit": "ms per call, min of %d windows of %d back-to-back calls, host side included" % (WINDOWS, CALLS), "model": MODEL,
           "arms": {"fused": "attach_codec: vbx_pack_phoneme_latent (training: with d proj_in.weight / bias)",
                    "linear": "codec-free predictor fed F.linear(latents) (training: without d proj_in, that path has none)",
                    "plain": "codec-free predictor fed a ready [B, S, dim] condition (the parent commit's path)"}}
    for L in LATENTS:
        plain = vbx.DurationPredictor(**MODEL).to(dev)
        fused = vbx.DurationPredictor(**MODEL).to(dev).attach_codec(ToyCodec(L))
        fused.load_state_dict({**plain.state_dict(), **{k: v for k, v in fused.state_dict().items() if k.startswith("proj_in.")}})
        pw, pb = fused.proj_in.weight.detach(), fused.proj_in.bias.detach()
        for B, n in SHAPES:
            lat = torch.randn(B, n, L, device=dev)
            cond = torch.randn(B, n, MODEL["dim"], device=dev)
            ids = torch.randint(0, MODEL["num_phoneme_tokens"], (B, n), device=dev)
            if B > 1:
                ids[B // 2:, (3 * n) // 4:] = -1
            cond_mask = torch.rand(B, n, device=dev) < 0.7
            target = torch.randint(1, 12, (B, n), device=dev).float()

            def run(arm, train):
                dp = fused if arm == "fused" else plain
                c = lat if arm == "fused" else (F.linear(lat, pw, pb) if arm == "linear" else cond)
                if not train:
                    return dp(cond=c, phoneme_ids=ids, cond_mask=cond_mask)
                for q in dp.parameters():
                    q.grad = None
                dp(cond=c, phoneme_ids=ids, cond_mask=cond_mask, target=target).backward()

            row = {}
            for mode, train in (("forward", False), ("forward_backward", True)):
                fused.train(train)
                plain.train(train)
                arms = ("fused", "linear", "plain")
                for arm in arms:  # warm up: allocator, weight packing, engines
                    run(arm, train)
                    run(arm, train)
                best = {arm: float("inf") for arm in arms}
                for _ in range(WINDOWS):
                    for arm in arms:  # the arms alternate
                        best[arm] = min(best[arm], window(lambda: run(arm, train)))
                row[mode] = {arm: round(v, 4) for arm, v in best.items()}
            res[f"L{L}_{B}x{n}"] = row
            print(f"L={L} {B}x{n}", json.dumps(row), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
