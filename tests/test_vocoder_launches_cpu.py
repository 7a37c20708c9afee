"""CPU (-m "not gpu"): the host side of HiFiGANGenerator and BigVGANGenerator hands the library what it handed it on the commit before
the two generators' shared code moved into one base class, and the weight-norm fold of every module that has one is the documented
expression bit for bit.

 * tests/golden/vocoder_launches_parent.json (tests/golden/make_vocoder_launches_parent.py, run on that parent) holds, per case, the
   launches of one gen._generate(mel) -- entry names, scalars, which buffer feeds which argument, shapes and dtypes -- and the SHA-256 of
   the mel and of every packed operand.  The cases are rebuilt here from the maker's cases() and compared, case by case.  With the
   library itself unchanged, the same operands through the same launches are the same bits on the device.
 * Under snake_logscale alpha and 1 / (beta + 1e-9) pass through exp, which need not agree between hosts: that case leaves them out
   of the hashes and compares them with torch.exp evaluated here.
 * folded() of every weight_g / weight_v layer of HiFiGANGenerator, BigVGANGenerator, SEANetEncoder and SEANetDecoder -- convolutions in
   all four, transposed convolutions in the three that have one -- is torch.equal to g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
   evaluated here, on values whose v does not have norm g."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_vocoder_launches_parent as M  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocoder_launches_parent.json")) as fh:
    PARENT = json.load(fh)["cases"]
CASES = M.cases()


def test_every_recorded_case_is_run():
    assert [name for name, _, _ in CASES] == list(PARENT)
    counts = {name[:2]: len(rec["launches"]) for name, rec in PARENT.items()}
    assert counts["H1"] == 23 and counts["B1"] == counts["B5"] == 41, counts  # the whole sequences, not a stub of them


@pytest.mark.parametrize("name,make,skip_exp", CASES, ids=[name.split()[0] for name, _, _ in CASES])
def test_launches_and_operands_equal_the_parent(name, make, skip_exp):
    gen = make()
    got, want = M.record(gen, M.mel_for(gen), skip_exp), PARENT[name]
    assert len(got["launches"]) == len(want["launches"])
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, f"launch {i}"
    assert list(got["sha256"]) == list(want["sha256"])  # the same operands, in the same structure
    for path, h in want["sha256"].items():
        assert got["sha256"][path] == h, path
    if skip_exp:  # what the hashes left out: every Activation1d's alpha and 1 / (beta + 1e-9), block by block, then activation_post
        ops = gen.packed_ops()
        acts = [a for stage in ops["stages"] for block in stage["blocks"] for a1, _, a2, _ in block for a in (a1, a2)] + [ops["post"]["act"]]
        mods = [a for rb in gen.resblocks for a in rb.activations] + [gen.activation_post]
        assert len(acts) == len(mods) == 2 * 3 * 3 * 2 + 1  # stages x blocks x dilations x two per pair, and activation_post
        for a, m in zip(acts, mods):
            assert torch.equal(a["alpha"], torch.exp(m.act.alpha.detach().float()))
            assert torch.equal(a["invb"], 1.0 / (torch.exp(m.act.beta.detach().float()) + 1e-9))


# ------------------------------------------------------------------------------------ the weight-norm fold, bit for bit
def _fill(module):
    """every parameter from the closed form: weight_g in 0.8 .. 1.2, the rest 0.3 u (|v| is about 0.09 sqrt(fan), 1 only at a fan of 133)"""
    start = 0
    with torch.no_grad():
        for name, p in module.named_parameters():
            v = M.u(tuple(p.shape), 1.0, start)
            p.copy_(1.0 + 0.4 * v if name.endswith("weight_g") else 0.3 * v)
            start += p.numel()
    return module


def _modules():
    import bigvgan_ref as R
    import hifigan_ref as H
    import voicebox_pytorch_amd as vbx

    small = dict(n_filters=16, ratios=(5, 2), dimension=32)
    return [("HiFiGANGenerator", vbx.HiFiGANGenerator(**H.SMALL), "{}", True), ("BigVGANGenerator", vbx.BigVGANGenerator(**R.SMALL), "{}", True),
            ("SEANetEncoder", vbx.SEANetEncoder(**small), "{}.conv.conv", False), ("SEANetDecoder", vbx.SEANetDecoder(**small), "{}.conv.conv", True)]


def test_fold_is_the_documented_expression_bit_for_bit():
    for who, module, inner, has_transposed in _modules():
        sd = _fill(module).state_dict()
        kinds = set()
        for path, w in module.folded_weights().items():
            key = inner.format(path)
            if f"{key}.weight_g" not in sd:
                key = f"{path}.convtr.convtr"  # SEANet's transposed convolution
            g, v = sd[f"{key}.weight_g"].float(), sd[f"{key}.weight_v"].float()
            norm = v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
            assert float((norm - 1).abs().max()) > 1e-2 and float((g / norm - 1).abs().max()) > 1e-2, (who, path)  # neither |v| = 1 nor |v| = g
            assert w.dtype == torch.float32 and torch.equal(w, g * v / norm), (who, path)
            kinds.add("transposed" if key.endswith("convtr") or path.startswith("ups.") else "conv")
        assert kinds == ({"conv", "transposed"} if has_transposed else {"conv"}), (who, kinds)
