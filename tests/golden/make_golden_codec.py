"""Generates the codec-latent fixtures by running the UNMODIFIED reference (oracle/ref_loader.py) with the weight-free test codec
of tests/toy_codec.py as its audio_enc_dec:

    python tests/golden/make_golden_codec.py   ->  tests/golden/{small_codec,small_codec_text}{,_grads}.pt   (tensors only)

(the gradients of a fixture live in a file of their own, `<name>_grads.pt`, so that every committed file stays below 1 MiB)

The loader's torchaudio stub returns None for `resample`; at equal rates the library returns its input, so the loaded module's
`resample` is bound to the identity here.  RNG protocol as make_golden.py: the draws of a training step are replayed under the
same seed and stored beside the results."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_loader  # noqa: E402
from toy_codec import ToyCodec  # noqa: E402

TIME_HIDDEN, FF_MULT = 64, 2  # keep the adaLN projections and the FeedForward (and with them each fixture) small


def load_ref():
    ref = ref_loader.load_reference()
    ref.resample = lambda x, a, b: x  # equal rates: the identity
    return ref


def replay_draws(x1, seed):
    torch.manual_seed(seed)
    b = x1.shape[0]
    x0 = torch.randn_like(x1)
    times = torch.rand((b,), dtype=x1.dtype)
    frac = torch.zeros((b,)).float().uniform_(0.7, 1.0)
    rand = torch.zeros_like(frac).float().uniform_(0, 1)
    return x0, times, frac, rand


def condition(vb, seed, null_cond=False):
    """well-conditioned weights, the recipe of the other small fixtures"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in vb.named_parameters():
            if ".to_gamma." in name or ".to_beta." in name:
                prm.add_(torch.randn(prm.shape, generator=g) * 0.05)
            if name.endswith("final_norm.gamma"):
                prm.add_(torch.randn(prm.shape, generator=g) * 0.1)
            if name.endswith("q_norm.gamma") or name.endswith("k_norm.gamma"):
                prm.add_(torch.randn(prm.shape, generator=g) * 0.1)
                prm.mul_(0.25)
        if null_cond:
            vb.null_cond.add_(torch.randn(vb.null_cond.shape, generator=g) * 0.3)


def _save(out, name):
    torch.save({k: v for k, v in out.items() if k != "grads"}, os.path.join(HERE, name + ".pt"))
    torch.save(out["grads"], os.path.join(HERE, name + "_grads.pt"))


def build_small_codec(ref):
    codec = ToyCodec(100)
    torch.manual_seed(0)
    vb = ref.VoiceBox(dim=64, audio_enc_dec=codec, num_cond_tokens=500, depth=2, dim_head=64, heads=2, condition_on_text=False,
                      time_hidden_dim=TIME_HIDDEN, ff_mult=FF_MULT, num_register_tokens=16)
    condition(vb, 126)
    return codec, vb


def gen_small_codec(ref, save=True):
    """latent 100 into dim 64: proj_in Linear(100, 64), to_embed Linear(128, 64), to_pred Linear(64, 100); trained from a wave."""
    codec, vb = build_small_codec(ref)
    wrapper = ref.ConditionalFlowMatcherWrapper(voicebox=vb)
    state = {k: v.detach().clone() for k, v in vb.state_dict().items()}
    assert state["proj_in.weight"].shape == (64, 100) and state["to_embed.weight"].shape == (64, 128)
    assert state["to_pred.weight"].shape == (100, 64) and state["null_cond"].shape == (64,)
    wave = torch.randn(2, 640, generator=torch.Generator().manual_seed(73))
    with torch.no_grad():
        lat = codec.encode(wave)
    x0, times, frac, rand = replay_draws(lat, seed=96)
    torch.manual_seed(96)
    loss = wrapper(wave)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in vb.named_parameters() if p.grad is not None}
    assert float(grads["proj_in.weight"].abs().max()) > 0 and float(grads["proj_in.bias"].abs().max()) > 0
    # mixed call: latents in, the condition as a wave
    wave_c = torch.randn(2, 640, generator=torch.Generator().manual_seed(74))
    lat1 = torch.randn(2, 40, 100, generator=torch.Generator().manual_seed(75))
    vb.zero_grad()
    torch.manual_seed(96)
    loss_mixed = wrapper(lat1, cond=wave_c)
    vb.eval()
    tt = torch.tensor([0.25, 0.8])
    with torch.no_grad():
        cond = codec.encode(wave_c)
        pred = vb(lat1, times=tt, cond_token_ids=None, cond=cond, cond_drop_prob=0.0)
    torch.manual_seed(32)
    y0 = torch.randn_like(cond)
    torch.manual_seed(32)
    s5 = wrapper.sample(cond=wave_c, steps=5, decode_to_audio=False)
    torch.manual_seed(32)
    s5_wave = wrapper.sample(cond=wave_c, steps=5)
    out = dict(latent_dim=100, time_hidden_dim=TIME_HIDDEN, ff_mult=FF_MULT, state=state, wave=wave, x0=x0, times=times, frac=frac, rand=rand,
               loss=loss.detach(), grads=grads, wave_cond=wave_c, lat1=lat1, loss_mixed=loss_mixed.detach(), eval_times=tt, pred=pred,
               y0=y0, sample5=s5, sample5_wave=s5_wave)
    if save:
        _save(out, "small_codec")
        print("small_codec: loss", float(loss), "mixed", float(loss_mixed), "pred", tuple(pred.shape), "sample", tuple(s5.shape),
              tuple(s5_wave.shape))
    return out


def gen_small_codec_text(ref, save=True):
    """latent 128 into dim 64, text-conditioned with classifier-free drop (the null_cond branch) and sample(cond=None)."""
    codec = ToyCodec(128)
    torch.manual_seed(0)
    vb = ref.VoiceBox(dim=64, audio_enc_dec=codec, num_cond_tokens=50, dim_cond_emb=48, depth=2, dim_head=64, heads=2,
                      condition_on_text=True, time_hidden_dim=TIME_HIDDEN, ff_mult=FF_MULT, num_register_tokens=16)
    condition(vb, 127, null_cond=True)
    wrapper = ref.ConditionalFlowMatcherWrapper(voicebox=vb, cond_drop_prob=0.5)
    state = {k: v.detach().clone() for k, v in vb.state_dict().items()}
    assert state["proj_in.weight"].shape == (64, 128) and state["to_embed.weight"].shape == (64, 176)
    b, n = 3, 40
    g = torch.Generator().manual_seed(78)
    wave = torch.randn(b, n * 16, generator=g)
    ids = torch.randint(0, 50, (b, n), generator=g)
    with torch.no_grad():
        lat = codec.encode(wave)
    x0, times, frac, rand = replay_draws(lat, seed=57)
    drop = torch.zeros((b,)).float().uniform_(0, 1) < 0.5  # prob_mask_like: the draw after the span-mask draws
    assert bool(drop.any()) and not bool(drop.all()), drop
    torch.manual_seed(57)
    loss = wrapper(wave, semantic_token_ids=ids)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in vb.named_parameters() if p.grad is not None}
    vb.eval()
    torch.manual_seed(5)
    y0 = torch.randn(b, n, 128)
    torch.manual_seed(5)
    s3 = wrapper.sample(cond=None, semantic_token_ids=ids, steps=3, cond_scale=1.3, decode_to_audio=False)
    torch.manual_seed(5)
    s3_wave = wrapper.sample(cond=wave, semantic_token_ids=ids, steps=3, cond_scale=1.3)
    out = dict(latent_dim=128, time_hidden_dim=TIME_HIDDEN, ff_mult=FF_MULT, state=state, wave=wave, ids=ids, x0=x0, times=times, frac=frac, rand=rand,
               drop=drop, loss=loss.detach(), grads=grads, y0=y0, sample3_nocond=s3, sample3_wave=s3_wave)
    if save:
        _save(out, "small_codec_text")
        print("small_codec_text: loss", float(loss), "drop", drop.tolist(), "sample", tuple(s3.shape), tuple(s3_wave.shape))
    return out


if __name__ == "__main__":
    ref = load_ref()
    which = sys.argv[1:] or ["small_codec", "small_codec_text"]
    for w in which:
        {"small_codec": gen_small_codec, "small_codec_text": gen_small_codec_text}[w](ref)
