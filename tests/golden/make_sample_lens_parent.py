"""Writes tests/golden/sample_lens_parent.json: one SHA-256 of the raw bytes of ConditionalFlowMatcherWrapper.sample()'s output per
case, recorded on the commit BEFORE sample() learned lens= / length_bucket=, together with the toolchain that produced the bits
(torch.version.hip, the `HIP version` line of hipcc --version).  With lens=None the sampler must keep its launch sequence, so
tests/test_sample_lens_gpu.py rebuilds the same calls from cases() and compares every hash.  One MI355X.

    python tests/golden/make_sample_lens_parent.py [OUT.json]

Inputs are the goldens' own (small_wc: cond, y0; small_text: cond, y0, ids_n), nothing is drawn.  The cases:

  small_wc midpoint steps5 eager      the un-captured interval
  small_wc midpoint steps5 graph      the captured interval
  small_text guided steps3 graph      text-conditioned, classifier-free guidance at cond_scale 1.3 (two forwards per evaluation)
  small_wc dopri5 graph               the adaptive solver: the error norm and the controller
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "sample_lens_parent.json")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda"


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def toolchain():
    """(torch.version.hip, the `HIP version` line of hipcc --version or why there is none)"""
    spec = importlib.util.spec_from_file_location("vbx_build", os.path.join(ROOT, "voicebox-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    try:
        out = subprocess.run([build._hipcc(), "--version"], capture_output=True, text=True, timeout=60).stdout
        line = next((l.strip() for l in out.splitlines() if l.startswith("HIP version")), "hipcc --version: no `HIP version` line")
    except (OSError, subprocess.SubprocessError) as e:
        line = f"hipcc --version failed: {type(e).__name__}"
    return str(torch.version.hip), line


def _golden(name):
    return torch.load(os.path.join(HERE, name + ".pt"), map_location="cpu", weights_only=False)


def _wc_case(method, steps, use_graph):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g = _golden("small_wc")
    vb = vbx.VoiceBox(dim=g["cfg"]["dim"], num_cond_tokens=500, depth=g["cfg"]["depth"], dim_head=64, heads=g["cfg"]["heads"],
                      condition_on_text=False)
    vb.load_state_dict(g["state"], strict=False)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(DEV), torchdiffeq_ode_method=method)
    with rng_override(y0=g["y0"]):
        return wrapper.sample(cond=g["cond"].to(DEV), steps=steps, use_graph=use_graph)


def _text_case():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g = _golden("small_text")
    vb = vbx.VoiceBox(dim=64, num_cond_tokens=50, dim_cond_emb=48, depth=2, dim_head=64, heads=2, condition_on_text=True)
    vb.load_state_dict(g["state"], strict=False)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(DEV))
    with rng_override(y0=g["y0"]):
        return wrapper.sample(cond=g["cond"].to(DEV), semantic_token_ids=g["ids_n"].to(DEV), steps=3, cond_scale=1.3, use_graph=True)


def cases():
    """(name, thunk -> output tensor on the device), in a fixed order"""
    return [("small_wc midpoint steps5 eager", lambda: _wc_case("midpoint", 5, False)),
            ("small_wc midpoint steps5 graph", lambda: _wc_case("midpoint", 5, True)),
            ("small_text guided steps3 graph", _text_case),
            ("small_wc dopri5 graph", lambda: _wc_case("dopri5", 3, True))]


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
    rec = {"note": "sha256 of the raw bytes of sample()'s output per case, recorded on the parent of the commit that introduced lens= "
                   "and length_bucket=; produced by tests/golden/make_sample_lens_parent.py on one MI355X",
           "torch_version_hip": hip, "hipcc_version": hipcc, "sha256": hashes()}
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(f"{len(rec['sha256'])} cases -> {path}")


if __name__ == "__main__":
    main()
