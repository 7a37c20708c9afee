"""Writes tests/golden/vocoder_launches_parent.json: what one HiFiGANGenerator / BigVGANGenerator call hands to the library, recorded
on the commit BEFORE the two generators' host code moved into one base class.  A call's result is decided by which entries are
launched with which scalars, how the buffers feed each other, and the bytes of the operands; all three are observed here on CPU
tensors, with _lib.call and _lib.current_stream replaced for the duration of one gen._generate(mel).  No GPU, no library.
tests/test_vocoder_launches_cpu.py runs cases() on the current tree and requires equality, case by case.

    python tests/golden/make_vocoder_launches_parent.py [OUT.json]

Per case: `launches`, one string per launch, entry(arg, ...) with None, an int, repr(float), or for a tensor t<index of first
appearance>:<shape>:<dtype>; and `sha256`, the hash of the bytes of the float32 mel and of every tensor in gen.packed_ops(), by its
path there.  No RNG anywhere: every input is the u(i) of make_codec_kernels_parent.py.  State dicts are in the PLAIN `weight` layout,
so that no reduction enters the hashed bytes: packing is then permutes, concatenations and one fp32 -> fp16 rounding, the same on
every machine.  Under snake_logscale alpha and 1 / (beta + 1e-9) pass through exp, which is not: that case leaves them out of the
hashes, and the test compares them with torch.exp evaluated beside it.

The cases, all at B = 2 and 5 frames, the smallest shapes that reach every branch of the host code:

  H1  HiFi-GAN hifigan_ref.SMALL, defaults: every residual pair is one fused launch
  H2  the same with fuse_max_channels = 8: the 16-wide stage as two launches with the residual in the second, the 8-wide one fused
  H3  hifigan_ref.SMALL2, input_log=True: ResBlock2, 20 mels padded to 24
  H4  one stage, one block, one dilation, one mel: xs has one entry, both spare inputs are None
  B1  BigVGAN bigvgan_ref.SMALL with snake_logscale=False, defaults: every residual convolution is vbx_bigvgan_conv
  B2  the same with fuse_act_max_channels = 0: vbx_bigvgan_act + vbx_hifigan_conv with act = 0 and slope 1.0
  B3  as B1 with rates (2, 4), kernels (4, 8) and the instance's FUSE_ACT_MAX_ELEMENTS = 320: the first stage (320 elements) fused,
      the second (640) not
  B4  bigvgan_ref.SMALL2: AMPBlock2, snake, clamp, no final bias (None in the post launch)
  B5  bigvgan_ref.SMALL as is (snake_logscale=True)
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "vocoder_launches_parent.json")
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_codec_kernels_parent import u  # noqa: E402  (the closed-form inputs)

B, FRAMES = 2, 5
EXP_KEYS = ("alpha", "invb")  # what passes through exp under snake_logscale


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def plain_state(layout, acts=(), beta=False, final_bias=True):
    """a state dict in the plain `weight` layout from the closed form: weights 2 u / sqrt(fan), biases 0.2 u, alpha and beta
    1.5 + u (in 1 .. 2: positive as they are and as logarithms), the two filters 0.3 u -- each tensor counted on from where the last ended"""
    sd, start = {}, 0

    def nxt(shape, scale, offset=0.0):
        nonlocal start
        t = u(shape, scale, start) + offset
        start += t.numel()
        return t

    for p, kind, ci, co, k, _ in layout:
        sd[f"{p}.weight"] = nxt((ci, co, k) if kind == "convtr" else (co, ci, k), 2.0 / (ci * k) ** 0.5)
        if p != "conv_post" or final_bias:
            sd[f"{p}.bias"] = nxt((co,), 0.2)
    for p, c in acts:
        sd[f"{p}.act.alpha"] = nxt((c,), 1.0, 1.5)
        if beta:
            sd[f"{p}.act.beta"] = nxt((c,), 1.0, 1.5)
        sd[f"{p}.upsample.filter"], sd[f"{p}.downsample.lowpass.filter"] = nxt((1, 1, 12), 0.3), nxt((1, 1, 12), 0.3)
    return sd


def hifigan(cfg, set_attrs=(), **kw):
    import hifigan_ref as H
    import voicebox_pytorch_amd as vbx

    gen = vbx.HiFiGANGenerator(**cfg, **kw)
    gen.load_state_dict(plain_state(H.layout(cfg)))
    for name, value in set_attrs:
        setattr(gen, name, value)
    return gen.eval()


def bigvgan(cfg, set_attrs=()):
    import bigvgan_ref as R
    import voicebox_pytorch_amd as vbx

    gen = vbx.BigVGANGenerator(**cfg)
    gen.load_state_dict(plain_state(R.layout(cfg), R.act_layout(cfg), cfg["activation"] == "snakebeta", cfg["use_bias_at_final"]))
    for name, value in set_attrs:
        setattr(gen, name, value)
    return gen.eval()


def cases():
    """(name, thunk -> generator, whether alpha / invb stay out of the hashes), in a fixed order"""
    import bigvgan_ref as R
    import hifigan_ref as H

    h4 = dict(n_mels=1, upsample_initial_channel=16, upsample_rates=(2,), upsample_kernel_sizes=(4,), resblock="1",
              resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),))
    b1 = dict(R.SMALL, snake_logscale=False)
    b3 = dict(b1, upsample_rates=(2, 4), upsample_kernel_sizes=(4, 8))
    return [("H1 hifigan SMALL", lambda: hifigan(H.SMALL), False),
            ("H2 hifigan SMALL fuse_max_channels 8", lambda: hifigan(H.SMALL, [("fuse_max_channels", 8)]), False),
            ("H3 hifigan SMALL2 input_log", lambda: hifigan(H.SMALL2, input_log=True), False),
            ("H4 hifigan one stage one block one mel", lambda: hifigan(h4), False),
            ("B1 bigvgan SMALL linear", lambda: bigvgan(b1), False),
            ("B2 bigvgan SMALL linear fuse_act_max_channels 0", lambda: bigvgan(b1, [("fuse_act_max_channels", 0)]), False),
            ("B3 bigvgan rates 2 4 FUSE_ACT_MAX_ELEMENTS 320", lambda: bigvgan(b3, [("FUSE_ACT_MAX_ELEMENTS", 320)]), False),
            ("B4 bigvgan SMALL2", lambda: bigvgan(R.SMALL2), False),
            ("B5 bigvgan SMALL logscale", lambda: bigvgan(R.SMALL), True)]


def mel_for(gen):
    return u((B, gen.n_mels, FRAMES), 4.0, 9 << 20)


def op_tensors(ops, path="ops"):
    """(path, tensor) of every tensor in a packed_ops() structure, in its own order"""
    if torch.is_tensor(ops):
        yield path, ops
    elif isinstance(ops, dict):
        for k, v in ops.items():
            yield from op_tensors(v, f"{path}.{k}")
    elif isinstance(ops, (list, tuple)):
        for i, v in enumerate(ops):
            yield from op_tensors(v, f"{path}.{i}")


def record(gen, mel, skip_exp=False):
    """one gen._generate(mel) on CPU tensors with the library's call replaced: dict(launches, sha256)"""
    from voicebox_pytorch_amd import _lib

    seen, keep, launches = {}, [], []  # keep: a reference to every tensor argument, so that no address comes twice

    def arg(a):
        if a is None or isinstance(a, int):
            return str(a)
        if isinstance(a, float):
            return repr(a)
        assert torch.is_tensor(a), type(a)
        keep.append(a)
        index = seen.setdefault(a.data_ptr(), len(seen))
        return f"t{index}:{'x'.join(str(s) for s in a.shape)}:{str(a.dtype).replace('torch.', '')}"

    def call(name, *args):
        launches.append(f"{name}({', '.join(arg(a) for a in args)})")
        return 0

    saved = _lib.call, _lib.current_stream
    _lib.call, _lib.current_stream = call, lambda: 0
    try:
        with torch.inference_mode():
            gen._generate(mel)
    finally:
        _lib.call, _lib.current_stream = saved
    assert keep[0].dtype == torch.float32 and tuple(keep[0].shape) == tuple(mel.shape)  # the first argument of the first launch
    hashes = {"mel": sha(keep[0])}
    for path, t in op_tensors(gen.packed_ops()):
        if not (skip_exp and path.rsplit(".", 1)[1] in EXP_KEYS):
            assert path not in hashes
            hashes[path] = sha(t)
    return dict(launches=launches, sha256=hashes)


def records():
    out = {}
    for name, make, skip_exp in cases():
        gen = make()
        assert name not in out
        out[name] = record(gen, mel_for(gen), skip_exp)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    rec = {"note": "per case the launches of one gen._generate(mel) on CPU tensors and the sha256 of the mel and of every packed operand, "
                   "recorded on the parent of the commit that introduced the generators' shared base class; produced by "
                   "tests/golden/make_vocoder_launches_parent.py, no GPU",
           "cases": records()}
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(f"{len(rec['cases'])} cases, {sum(len(c['launches']) for c in rec['cases'].values())} launches -> {path}")


if __name__ == "__main__":
    main()
