"""Times of DurationPredictor training on one MI355X against the same function in eager PyTorch:
    python tools/duration_train_times.py [OUT.json]        (default: profiles/duration_train_times.json)

Two arms alternate in one process, window by window: this package's DurationPredictor in train() mode, and
oracle.restate.duration_predictor_forward in fp32 on the device with the masked L1 of tests/duration_train_ref.py under torch
autograd, over the same parameters.  The aligner part (Aligner, maximum_path, ForwardSumLoss) goes through this package in both
arms.  Per shape: forward + backward of the given-durations branch and of the aligner branch with return_aligned_phoneme_ids=True.
A window is 10 back-to-back calls between two host synchronisations, wall clock, host side included; the figure is the minimum of
five windows per call (the method of tools/aligner_times.py)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voicebox_pytorch_amd as vbx  # noqa: E402
from oracle import restate  # noqa: E402
import duration_train_ref as R  # noqa: E402

dev = "cuda"
MODEL = dict(dim=512, depth=10, heads=8, dim_head=64, dim_phoneme_emb=512, num_phoneme_tokens=256)
SHAPES = [(8, 200, 1024), (1, 60, 301)]  # B, n (phonemes), T (mel frames)
CALLS, WINDOWS = 10, 5


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / CALLS * 1e3


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "duration_train_times.json")
    torch.manual_seed(0)
    res = {"unit": "ms per forward + backward, min of %d windows of %d back-to-back calls, host side included" % (WINDOWS, CALLS),
           "model": MODEL, "arms": {"package": "DurationPredictor.train()(...) + backward",
                                    "torch": "oracle.restate.duration_predictor_forward in fp32 + masked L1 + autograd; aligner part "
                                             "through this package"}}
    cfg = restate.Cfg(dim=MODEL["dim"], depth=MODEL["depth"], heads=MODEL["heads"], dim_head=64, num_register_tokens=0, qk_norm=True)
    for B, n, T in SHAPES:
        dp = vbx.DurationPredictor(**MODEL).to(dev).train()
        aligner = dp.attach_aligner()
        p = {k: v for k, v in dp.state_dict(keep_vars=True).items() if not k.startswith("aligner.")}
        cond = torch.randn(B, n, MODEL["dim"], device=dev)
        ids = torch.randint(0, MODEL["num_phoneme_tokens"], (B, n), device=dev)
        plen = torch.full((B,), n, device=dev, dtype=torch.int64)
        plen[B // 2:] = (3 * n) // 4 if B > 1 else n
        ids = torch.where(torch.arange(n, device=dev)[None] < plen[:, None], ids, torch.full_like(ids, -1))
        cond_mask = torch.rand(B, n, device=dev) < 0.7
        target = torch.randint(1, 12, (B, n), device=dev).float()
        mel = torch.randn(B, T, dp.aligner_kwargs["dim_in"], device=dev)
        mlen = torch.full((B,), T, device=dev, dtype=torch.int64)
        pmask = (ids != -1)[:, None].to(torch.int32)
        mmask = torch.ones(B, 1, T, device=dev, dtype=torch.int32)
        sam = ids != -1
        params = [q for q in dp.parameters() if q.requires_grad]

        def zero():
            for q in params:
                q.grad = None

        def package(branch):
            zero()
            if branch == "given":
                loss = dp(cond=cond, phoneme_ids=ids, target=target, cond_mask=cond_mask)
            else:
                loss = dp(cond=cond, phoneme_ids=ids, cond_mask=cond_mask, mel=mel, phoneme_len=plen, mel_len=mlen, phoneme_mask=pmask,
                          mel_mask=mmask, return_aligned_phoneme_ids=True)
            loss.backward()

        def torch_arm(branch):
            zero()
            with torch.device(dev):  # the restatement builds its position tables with the default device
                d = restate.duration_predictor_forward(p, cfg, cond, ids, cond_mask)
            t, extra = target, 0.0
            if branch == "aligner":
                emb = dp.to_phoneme_emb.weight[ids.clamp(min=0)]
                t, _, logprob, _ = dp.forward_aligner(emb, pmask, mel, mmask)
                extra = vbx.ForwardSumLoss()(logprob, plen, mlen)
            (R.masked_l1(d, t, cond_mask, sam) + extra).backward()

        row = {}
        for branch in ("given", "aligner"):
            arms = {"package": package, "torch": torch_arm}
            for arm in arms:  # warm up: allocator, weight packing, engines
                arms[arm](branch)
                arms[arm](branch)
            best = {arm: float("inf") for arm in arms}
            for _ in range(WINDOWS):
                for arm in arms:  # the arms alternate
                    best[arm] = min(best[arm], window(lambda: arms[arm](branch)))
            row[branch] = {arm: round(v, 4) for arm, v in best.items()}
        res[f"{B}x{n}_T{T}"] = row
        print(f"{B}x{n} T={T}", json.dumps(row), flush=True)
        del aligner
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
