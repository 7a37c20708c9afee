"""CPU (-m "not gpu"): voicebox_pytorch_amd.HiFiGANGenerator's host side and its yardstick tests/hifigan_ref.py.

 * the restatement equals, to 1e-12, an independent construction from nn.Conv1d / nn.ConvTranspose1d under
   torch.nn.utils.parametrizations.weight_norm in the published forward's order;
 * every state-dict layout loads to the same folded weights; from_checkpoint round-trips synthetic LOCAL files with and without config=;
 * every constructor refusal raises; the phase packing of the transposed weight reproduces F.conv_transpose1d;
 * PLANTED FAULTS: each of hifigan_ref.FAULTS moves the fp64 output by max |delta| / RMS far above the parity tolerance, which is
   DEFINED as one tenth of the smallest movement (hifigan_ref.parity_tolerance) and written, with every movement, into
   profiles/hifigan_parity.txt.  Parity with the HiFi-GAN library itself is UNPINNED."""
import json

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import hifigan_ref as H
import hifigan_tol as T


# ------------------------------------------------------------------------------------ the restatement against torch's own modules
class _Published(nn.Module):
    """HiFi-GAN's Generator as published, from torch's modules (fp64)"""

    def __init__(self, cfg):
        super().__init__()
        wn = nn.utils.parametrizations.weight_norm
        self.cfg, c = cfg, cfg["upsample_initial_channel"]
        self.conv_pre = wn(nn.Conv1d(cfg["n_mels"], c, 7, padding=3))
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
            self.ups.append(wn(nn.ConvTranspose1d(c, c // 2, k, u, padding=(k - u) // 2)))
            c //= 2
            for rk, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
                first = nn.ModuleList([wn(nn.Conv1d(c, c, rk, dilation=d, padding=(rk * d - d) // 2)) for d in ds])
                second = nn.ModuleList([wn(nn.Conv1d(c, c, rk, padding=(rk - 1) // 2)) for _ in ds]) if cfg["resblock"] == "1" else None
                self.resblocks.append(nn.ModuleList([first, second] if second is not None else [first]))
        self.conv_post = wn(nn.Conv1d(c, 1, 7, padding=3))

    def load(self, sd):
        nk, mods = len(self.cfg["resblock_kernel_sizes"]), {"conv_pre": self.conv_pre, "conv_post": self.conv_post}
        for i, up in enumerate(self.ups):
            mods[f"ups.{i}"] = up
        for n, rb in enumerate(self.resblocks):
            for m, c in enumerate(rb[0]):
                mods[f"resblocks.{n}.convs1.{m}" if len(rb) == 2 else f"resblocks.{n}.convs.{m}"] = c
            if len(rb) == 2:
                for m, c in enumerate(rb[1]):
                    mods[f"resblocks.{n}.convs2.{m}"] = c
        assert nk * len(self.ups) == len(self.resblocks)
        with torch.no_grad():
            for p, m in mods.items():
                m.parametrizations.weight.original0.copy_(sd[f"{p}.weight_g"])
                m.parametrizations.weight.original1.copy_(sd[f"{p}.weight_v"])
                m.bias.copy_(sd[f"{p}.bias"])
        return self

    def forward(self, x):
        nk = len(self.cfg["resblock_kernel_sizes"])
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            x = up(F.leaky_relu(x, 0.1))
            xs = None
            for j in range(nk):
                rb, h = self.resblocks[i * nk + j], x
                for m in range(len(rb[0])):
                    t = rb[0][m](F.leaky_relu(h, 0.1))
                    if len(rb) == 2:
                        t = rb[1][m](F.leaky_relu(t, 0.1))
                    h = t + h
                xs = h if xs is None else xs + h
            x = xs / nk
        return torch.tanh(self.conv_post(F.leaky_relu(x)))[:, 0]


@pytest.mark.parametrize("name", ["SMALL", "SMALL2"])
def test_restatement_equals_the_published_construction(name):
    cfg = getattr(H, name)
    sd = H.random_state(cfg, 0)
    mel = H.mels(2, cfg["n_mels"], 17, 1)
    ref = H.generate(sd, cfg, mel)
    with torch.no_grad():
        pub = _Published(cfg).double().load(sd)(mel.double())
    assert ref.shape == pub.shape == (2, 17 * H.hop(cfg))
    assert float((ref - pub).abs().max()) <= 1e-12
    rms = float(ref.pow(2).mean().sqrt())
    assert 0.3 <= rms <= 0.9, rms  # tanh is exercised, and not saturated everywhere
    if name == "SMALL":  # input_log: the log of the clamped amplitudes in front
        amp = H.mels(2, cfg["n_mels"], 17, 2, amplitude=True)
        with torch.no_grad():
            pub = _Published(cfg).double().load(sd)(torch.log(torch.clamp(amp.double(), min=1e-5)))
        assert float((H.generate(sd, cfg, amp, input_log=True) - pub).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------ planted faults and the tolerance
def test_planted_faults_move_the_output_and_set_the_tolerance():
    tol, moves, emu = T.parity_tolerance()
    lines = [f"tolerance (one tenth of the smallest planted fault's movement, max |delta| / RMS, fp64): {tol:.4e}"]
    for (name, fault), v in sorted(moves.items(), key=lambda kv: kv[1]):
        lines.append(f"  fault {fault:<12} config {name:<6} moves the output by {v:.4e}")
    for name, v in emu.items():
        lines.append(f"  emulated-precision restatement vs fp64, config {name:<6}: {v:.4e} ({tol / v:.1f} x inside the tolerance)")
    print("\n".join(lines))
    T.write_section("cpu", lines)
    assert {f for _, f in moves} == set(H.FAULTS)  # every fault was planted somewhere
    assert all(v >= 10 * tol * (1 - 1e-12) for v in moves.values())
    # what the contract's roundings alone cost must leave room for the kernels' fp32 summation order: at least half the tolerance
    assert all(v <= tol / 2 for v in emu.values()), (emu, tol)


# ------------------------------------------------------------------------------------ state dicts and files
def _generator(cfg, **kw):
    import voicebox_pytorch_amd as vbx

    return vbx.HiFiGANGenerator(**cfg, **kw)


def _same_folded(gen, sd, exact=False):
    got = gen.folded_weights()
    assert set(got) == {p for p, *_ in H.layout(H.SMALL if gen.resblock == "1" else H.SMALL2)}
    for p, w in got.items():
        ref = H.fold(sd, p, torch.float32)
        assert w.shape == ref.shape
        assert torch.equal(w, ref) if exact else float((w - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), p


@pytest.mark.parametrize("name", ["SMALL", "SMALL2"])
def test_state_dict_layouts(name):
    cfg = getattr(H, name)
    sd = H.random_state(cfg, 1, calibrate=False)
    gen = _generator(cfg)
    assert {k: tuple(v.shape) for k, v in gen.state_dict().items()} == H.expected_shapes(cfg)
    assert gen.hop_length == H.hop(cfg)
    gen.load_state_dict(sd)
    _same_folded(gen, sd)
    new = {}
    for k, v in sd.items():
        new[k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1")] = v
    gen2 = _generator(cfg)
    gen2.load_state_dict(new)
    _same_folded(gen2, sd)
    gen3 = _generator(cfg)
    gen3.load_state_dict({"generator": sd})
    _same_folded(gen3, sd)
    plain = {}
    for p, *_ in H.layout(cfg):
        plain[f"{p}.weight"], plain[f"{p}.bias"] = H.fold(sd, p, torch.float32), sd[f"{p}.bias"]
    gen4 = _generator(cfg)
    gen4.load_state_dict(plain)
    _same_folded(gen4, plain, exact=True)
    assert set(gen4.state_dict()) == set(plain)
    gen4.load_state_dict(sd)  # and back under weight norm
    assert set(gen4.state_dict()) == set(sd)
    with pytest.raises(RuntimeError):
        _generator(cfg).load_state_dict({k: v for k, v in sd.items() if not k.startswith("conv_post")})


def test_from_checkpoint_round_trips(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = H.random_state(H.SMALL, 2, calibrate=False)
    path = tmp_path / "generator_small.pt"
    torch.save({"generator": sd}, path)
    gen = vbx.HiFiGANGenerator.from_checkpoint(str(path))
    for key in ("n_mels", "upsample_initial_channel", "upsample_rates", "upsample_kernel_sizes", "resblock", "resblock_kernel_sizes",
                "resblock_dilation_sizes"):
        assert getattr(gen, key) == H.SMALL[key], key
    assert not gen.training and not gen.input_log
    _same_folded(gen, sd)
    # the dilations are in no shape: config= says them, as a dict or as a LOCAL json file (HiFi-GAN's config.json keys)
    cfgd = dict(resblock="1", upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=32, num_mels=16,
                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 2, 4], [1, 3, 5], [2, 6, 12]], segment_size=8192)
    gen = vbx.HiFiGANGenerator.from_checkpoint(str(path), config=cfgd, input_log=True)
    assert gen.resblock_dilation_sizes == ((1, 2, 4), (1, 3, 5), (2, 6, 12)) and gen.input_log
    cpath = tmp_path / "config.json"
    cpath.write_text(json.dumps(cfgd))
    gen = vbx.HiFiGANGenerator.from_checkpoint(str(path), config=str(cpath))
    assert gen.resblock_dilation_sizes == ((1, 2, 4), (1, 3, 5), (2, 6, 12))
    assert [c.dilation for c in gen.resblocks[2].convs1] == [2, 6, 12] and [c.dilation for c in gen.resblocks[2].convs2] == [1, 1, 1]
    for key, bad in (("upsample_rates", [4, 2]), ("resblock", "2"), ("num_mels", 80), ("resblock_kernel_sizes", [3, 7, 9]),
                     ("resblock_dilation_sizes", [[1, 3], [1, 3], [1, 3]])):
        with pytest.raises(ValueError):
            vbx.HiFiGANGenerator.from_checkpoint(str(path), config=dict(cfgd, **{key: bad}))
    # ResBlock2 without a config: V3's (1, 3) are ASSUMED -- this file was made with (1, 2) and (2, 6), and nothing can tell
    sd2 = H.random_state(H.SMALL2, 3, calibrate=False)
    torch.save(sd2, tmp_path / "g2.pt")
    gen = vbx.HiFiGANGenerator.from_checkpoint(str(tmp_path / "g2.pt"))
    assert gen.resblock == "2" and gen.resblock_dilation_sizes == ((1, 3), (1, 3)) and gen.upsample_rates == (4, 2) and gen.n_mels == 20
    gen = vbx.HiFiGANGenerator.from_checkpoint(str(tmp_path / "g2.pt"), config={"resblock_dilation_sizes": H.SMALL2["resblock_dilation_sizes"]})
    assert gen.resblock_dilation_sizes == H.SMALL2["resblock_dilation_sizes"]
    with pytest.raises(RuntimeError):
        vbx.HiFiGANGenerator.from_state_dict({"conv_pre.bias": torch.zeros(4)})


REFUSED = [dict(n_mels=0), dict(n_mels=513), dict(upsample_initial_channel=520), dict(upsample_initial_channel=2048),
           dict(upsample_initial_channel=64), dict(upsample_rates=(8, 8, 2, 2, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4, 4, 4)),
           dict(upsample_rates=(), upsample_kernel_sizes=()), dict(upsample_rates=(5, 8, 2, 2), upsample_kernel_sizes=(10, 16, 4, 4)),
           dict(upsample_rates=(10, 8, 2, 2), upsample_kernel_sizes=(20, 16, 4, 4)), dict(upsample_kernel_sizes=(16, 15, 4, 4)),
           dict(upsample_kernel_sizes=(16, 16, 4, 8)), dict(resblock="3"), dict(resblock_kernel_sizes=(3, 7, 13)),
           dict(resblock_kernel_sizes=(3, 4, 11)), dict(resblock_kernel_sizes=(1, 7, 11)), dict(resblock_dilation_sizes=((1, 3, 13),) * 3),
           dict(resblock_dilation_sizes=((0, 3, 5),) * 3), dict(resblock_dilation_sizes=((1, 3, 5, 7),) * 3),
           dict(resblock_dilation_sizes=((),) * 3), dict(resblock_kernel_sizes=(3, 5, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 4),
           dict(resblock_kernel_sizes=(), resblock_dilation_sizes=())]


@pytest.mark.parametrize("kw", REFUSED, ids=[",".join(f"{k}={v}" for k, v in kw.items())[:60] for kw in REFUSED])
def test_constructor_refusals(kw):
    import voicebox_pytorch_amd as vbx

    with pytest.raises(NotImplementedError, match="HiFiGANGenerator: .* is not built"):
        vbx.HiFiGANGenerator(**kw)


def test_accepted_edges_and_cpu_tensors():
    import voicebox_pytorch_amd as vbx

    vbx.HiFiGANGenerator(n_mels=100, upsample_initial_channel=1024, upsample_rates=(8,), upsample_kernel_sizes=(16,),
                         resblock_kernel_sizes=(11,), resblock_dilation_sizes=((12, 12, 12),))
    gen = vbx.HiFiGANGenerator(n_mels=1, upsample_initial_channel=256, upsample_rates=(2, 2, 2, 2, 2), upsample_kernel_sizes=(4,) * 5,
                               resblock="2", resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),))
    assert gen.hop_length == 32
    with pytest.raises(ValueError):
        vbx.HiFiGANGenerator(upsample_kernel_sizes=(16, 16, 4))
    with pytest.raises(vbx._lib.VbxError):
        gen(torch.zeros(1, 1, 4))
    with pytest.raises(ValueError):
        gen(torch.zeros(1, 2, 4))


@pytest.mark.parametrize("C,r", [(16, 2), (32, 4), (48, 8)])
def test_phase_packing_of_the_transposed_weight(C, r):
    """rows [a_j | a_{j-1}], j = 0 .. L, times the packed weight: row j's r * Co results are the output positions j r - r / 2 + p"""
    from voicebox_pytorch_amd.hifigan import pack_convtr_weight

    g = torch.Generator().manual_seed(C + r)
    Co, L = C // 2, 5
    w = torch.randn(C, Co, 2 * r, generator=g, dtype=torch.float64)
    x = torch.randn(2, C, L, generator=g, dtype=torch.float64)
    wp = pack_convtr_weight(w, r)
    assert wp.shape == (r * Co, 2 * C)
    a = F.pad(x.transpose(1, 2), (0, 0, 1, 1))  # [B, L + 2, C]: a_{-1} and a_L are zero
    rows = torch.cat([a[:, 1:], a[:, :-1]], dim=2)  # row j = [a_j | a_{j-1}], j = 0 .. L
    out = (rows @ wp.t()).reshape(2, L + 1, r, Co)
    got = out.reshape(2, (L + 1) * r, Co)[:, r // 2:r // 2 + L * r].transpose(1, 2)
    ref = F.conv_transpose1d(x, w, None, stride=r, padding=r // 2)
    assert got.shape == ref.shape == (2, Co, L * r)
    assert float((got - ref).abs().max()) <= 1e-12
