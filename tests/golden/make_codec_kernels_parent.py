"""Writes tests/golden/codec_kernels_parent.json: one SHA-256 of the raw output bytes per case of the codec kernels (csrc/mel.hip,
csrc/griffinlim.hip, csrc/seanet.hip), recorded on the commit BEFORE their shared parts moved into csrc/fft_lds.hpp and
sn_tile_product, together with the toolchain that produced the bits (torch.version.hip, the `HIP version` line of hipcc --version).
tests/test_codec_kernels_parent_gpu.py rebuilds the same inputs from cases() and compares every hash.  One MI355X.

    python tests/golden/make_codec_kernels_parent.py [OUT.json]

No RNG anywhere: element i (flat index, counted on from `start`) of every input is u(i) = ((i * 2654435761) mod 2^32) / 2^32 - 0.5
in fp64, scaled, then cast.  The cases are the smallest shapes that reach every path of the kernels:

  conv     the nine rows of CONVS in tests/test_seanet_gpu.py, B 2, L in {1, 3 stride + 1 (37 at stride 1), tile stride + 1}: all
           three position-block counts per work item, the clamped 16-position tile, the K-concatenated tail, dilation, fp32 output,
           the 138 KiB layer
  convtr   the five rows of CONVTRS in tests/test_seanet_dec_gpu.py, B 2, L in {1, 2, 17, tile + 1}
  logmel   LogMelCodec.encode at (n_fft, win, hop) in STFTS, B 2, T = 5 hop + 7 (6 frames: a partial last workgroup whose second
           transform carries nothing), log=True and once log=False
  gl       griffin_lim at the same three, B 2, 9 frames, an explicit phase, n_iter 0 (= the two launches of vbx_istft) and 2
  encoder / decoder   one whole SEANetEncoder and SEANetDecoder at the tests' SMALL_KW, B 2: the kernels that did not move and the
           order in which the operands are packed
"""
import hashlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "codec_kernels_parent.json")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STFTS = [(256, 160, 64), (1024, 640, 160), (2048, 1200, 300)]
DEV = "cuda"


def u(shape, scale, start=0, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(start, start + n, dtype=torch.int64)
    v = ((i * 2654435761) & 0xFFFFFFFF).double() / 2.0 ** 32 - 0.5
    return (v * scale).reshape(shape).to(dtype)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def toolchain():
    """(torch.version.hip, the `HIP version` line of hipcc --version or why there is none)"""
    spec_path = os.path.join(ROOT, "voicebox-pytorch_amd", "build.py")
    import importlib.util

    spec = importlib.util.spec_from_file_location("vbx_build", spec_path)
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    try:
        out = subprocess.run([build._hipcc(), "--version"], capture_output=True, text=True, timeout=60).stdout
        line = next((l.strip() for l in out.splitlines() if l.startswith("HIP version")), "hipcc --version: no `HIP version` line")
    except (OSError, subprocess.SubprocessError) as e:
        line = f"hipcc --version failed: {type(e).__name__}"
    return str(torch.version.hip), line


def _conv_case(C1, C2, Co, k, stride, dil, elu, out_f32, L):
    from voicebox_pytorch_amd import _lib

    B, K, Lout = 2, k * C1 + C2, -(-L // stride)
    x = u((B, L, C1), 2.0, 0, torch.float16).to(DEV)
    x2 = u((B, L, C2), 2.0, 1 << 20, torch.float16).to(DEV) if C2 else None
    w = u((Co, K), 2.0 / K ** 0.5, 2 << 20, torch.float16).to(DEV)
    bias = u((Co,), 0.2, 3 << 20).to(DEV)
    y = torch.zeros(B, Lout, Co, dtype=torch.float32 if out_f32 else torch.float16, device=DEV)
    _lib.call("vbx_seanet_conv", x, x2, w, bias, y, B, L, C1, C2, Co, k, stride, dil, int(elu), int(out_f32), _lib.current_stream())
    return y


def _convtr_case(C, r, L):
    from voicebox_pytorch_amd import _lib

    B, Co = 2, C // 2
    x = u((B, L, C), 2.0, 0, torch.float16).to(DEV)
    w = u((r * Co, 2 * C), 2.0 / (2 * C) ** 0.5, 2 << 20, torch.float16).to(DEV)  # the phase-packed layout as the kernel reads it
    bias = u((Co,), 0.2, 3 << 20).to(DEV)
    y = torch.zeros(B, L * r, Co, dtype=torch.float16, device=DEV)
    _lib.call("vbx_seanet_convtr", x, w, bias, y, B, L, C, r, _lib.current_stream())
    return y


def _logmel_case(n_fft, win, hop, log):
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec(log=log, n_fft=n_fft, win_length=win, hop_length=hop).to(DEV)
    return codec.encode(u((2, 5 * hop + 7), 1.0).to(DEV))


def _gl_case(n_fft, win, hop, n_iter):
    import math

    import voicebox_pytorch_amd as vbx

    nb, frames = n_fft // 2 + 1, 9
    mag = u((2, nb, frames), 2.0, 0, torch.float64).abs().float().to(DEV)
    phase = u((2, nb, frames), 2.0 * math.pi, 1 << 20, torch.float64).to(DEV)
    return vbx.griffin_lim(mag, n_fft=n_fft, win_length=win, hop_length=hop, n_iter=n_iter, momentum=0.99, phase=phase)


def _fill(module):
    """every parameter from the closed form, in named_parameters order: weight_g positive (1 + 0.4 u), the rest 0.5 u"""
    start = 0
    with torch.no_grad():
        for name, p in module.named_parameters():
            v = u(tuple(p.shape), 1.0, start)
            p.copy_(1.0 + 0.4 * v if name.endswith("weight_g") else 0.5 * v)
            start += p.numel()
    return module.to(DEV).eval()


def _encoder_case():
    import voicebox_pytorch_amd as vbx
    from test_seanet_gpu import SMALL_KW

    return _fill(vbx.SEANetEncoder(**SMALL_KW))(u((2, 131), 0.6, 7 << 20).to(DEV))


def _decoder_case():
    import voicebox_pytorch_amd as vbx
    from test_seanet_dec_gpu import SMALL_KW

    return _fill(vbx.SEANetDecoder(**SMALL_KW))(u((2, SMALL_KW["dimension"], 11), 6.0, 7 << 20).to(DEV))


def cases():
    """(name, thunk -> output tensor on the device), in a fixed order"""
    from test_seanet_dec_gpu import CONVTRS
    from test_seanet_gpu import CONVS
    from voicebox_pytorch_amd import _lib

    out = []
    for name, C1, C2, Co, k, stride, dil, elu, out_f32 in CONVS:
        tile = _lib.call_value("vbx_seanet_conv_tile", C1, C2, k, stride, dil)
        for L in sorted({1, 3 * stride + 1 if stride > 1 else 37, tile * stride + 1}):
            out.append((f"conv {name} L{L}", lambda a=(C1, C2, Co, k, stride, dil, elu, out_f32, L): _conv_case(*a)))
    for C, r in CONVTRS:
        tile = _lib.call_value("vbx_seanet_convtr_tile", C, r)
        for L in sorted({1, 2, 17, tile + 1}):
            out.append((f"convtr {C}-{C // 2} r{r} L{L}", lambda a=(C, r, L): _convtr_case(*a)))
    for n_fft, win, hop in STFTS:
        out.append((f"logmel {n_fft}/{win}/{hop} log", lambda a=(n_fft, win, hop, True): _logmel_case(*a)))
    out.append(("logmel 1024/640/160 power", lambda: _logmel_case(1024, 640, 160, False)))
    for n_fft, win, hop in STFTS:
        for n_iter in (0, 2):
            out.append((f"gl {n_fft}/{win}/{hop} iters{n_iter}", lambda a=(n_fft, win, hop, n_iter): _gl_case(*a)))
    out.append(("encoder small B2 T131", _encoder_case))
    out.append(("decoder small B2 F11", _decoder_case))
    return out


def hashes():
    out = {}
    for name, fn in cases():
        y = fn()
        torch.cuda.synchronize()
        assert name not in out, name
        out[name] = sha(y)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    hip, hipcc = toolchain()
    rec = {"note": "sha256 of the raw output bytes per case, recorded on the parent of the commit that introduced csrc/fft_lds.hpp and "
                   "sn_tile_product; produced by tests/golden/make_codec_kernels_parent.py on one MI355X",
           "torch_version_hip": hip, "hipcc_version": hipcc, "sha256": hashes()}
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(f"{len(rec['sha256'])} cases -> {path}")


if __name__ == "__main__":
    main()
