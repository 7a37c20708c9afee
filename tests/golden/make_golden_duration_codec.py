"""Generates the fixture of DurationPredictor over codec latents by running the UNMODIFIED reference (oracle/ref_loader.py) with the
weight-free test codec of tests/toy_codec.py as its audio_enc_dec:

    python tests/golden/make_golden_duration_codec.py   ->  tests/golden/duration_codec.pt   (tensors only)

The reference's DurationPredictor(audio_enc_dec=codec) has proj_in = Linear(latent_dim, dim) and applies it as the first line of
forward (voicebox_pytorch.py:627-630, :776): the mask, the classifier-free drop and curtail_or_pad follow it.  Two cases in the style
of gen_duration (make_golden.py): latent 100 with the condition SHORTER than the phoneme sequence, latent 128 with it LONGER; ragged
-1 padding, an explicit cond_mask, proj_in / null_cond / to_pred moved off their initial values.

Both models share every weight but proj_in (the second loads the first's), so the file stores those once: `common_state`, and per case
`state` = proj_in.* only.  tests/duration_codec_ref.py::fixture_cases puts the two together.  That keeps the file under 1 MiB."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_loader  # noqa: E402
from toy_codec import ToyCodec  # noqa: E402


def gen_duration_codec(ref):
    out, common = {}, None
    for name, L, S in (("latent100_short_cond", 100, 21), ("latent128_long_cond", 128, 40)):
        torch.manual_seed(9)
        dp = ref.DurationPredictor(audio_enc_dec=ToyCodec(L), num_phoneme_tokens=37, dim_phoneme_emb=32, dim=64, depth=2, dim_head=64,
                                   heads=2)
        g = torch.Generator().manual_seed(13 + L)
        with torch.no_grad():
            for n, prm in dp.named_parameters():
                if n.endswith("gamma"):
                    prm.add_(torch.randn(prm.shape, generator=g) * 0.1)
            dp.null_cond.copy_(torch.randn(64, generator=g) * 0.5)
            dp.proj_in.weight.add_(torch.randn(dp.proj_in.weight.shape, generator=g) * 0.05)
            dp.proj_in.bias.copy_(torch.randn(64, generator=g) * 0.5)  # far from 0: a masked row is 0, not the bias
            dp.to_pred[0].weight.mul_(4.0)
            dp.to_pred[0].bias.add_(2.5)
            if common is not None:  # every weight but proj_in is the first model's
                missing = dp.load_state_dict(common, strict=False)
                assert sorted(missing.missing_keys) == ["proj_in.bias", "proj_in.weight"] and not missing.unexpected_keys
        dp.eval()
        state = {k: v.detach().clone() for k, v in dp.state_dict().items()}
        if common is None:
            common = {k: v for k, v in state.items() if not k.startswith("proj_in.")}
        assert state["proj_in.weight"].shape == (64, L) and state["proj_in.bias"].shape == (64,)
        assert not any(k.startswith("audio_enc_dec.") for k in state)  # the test codec has no persistent state
        b, n = 3, 28
        ids = torch.randint(0, 37, (b, n), generator=g)
        ids[1, 20:] = -1
        ids[2, 9:] = -1
        cond = torch.randn(b, S, L, generator=g)
        cond_mask = torch.rand(b, S, generator=g) < 0.3
        with torch.no_grad():
            d1 = dp(cond=cond, phoneme_ids=ids, cond_mask=cond_mask)
            d_null = dp(cond=cond, phoneme_ids=ids, cond_mask=cond_mask, cond_drop_prob=1.0)
            d3, aligned = dp.forward_with_cond_scale(cond=cond, phoneme_ids=ids, cond_mask=cond_mask, cond_scale=3.0,
                                                     return_aligned_phoneme_ids=True)
        out[name] = dict(latent_dim=L, state={k: v for k, v in state.items() if k.startswith("proj_in.")}, ids=ids, cond=cond, cond_mask=cond_mask, d1=d1.clone(), d_null=d_null.clone(),
                         d3=d3.clone(), aligned=aligned.clone())
        print("duration_codec", name, d1[0, :6].tolist(), tuple(aligned.shape))
    torch.save(dict(common_state=common, cases=out), os.path.join(HERE, "duration_codec.pt"))


if __name__ == "__main__":
    gen_duration_codec(ref_loader.load_reference())
