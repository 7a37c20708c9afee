"""Host-side tests of voicebox_pytorch_amd.SEANetDecoder: the fp64 restatement tests/seanet_dec_ref.py against an independent
construction from torch's own modules, the state-dict layouts and loaders, the constructor limits, the phase packing of the
transposed convolution's weight, and that every planted fault of the restatement is far above the parity bound the GPU tests use.
Parity with the `encodec` library itself is UNPINNED."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import seanet_dec_ref as D
import seanet_ref as S
from test_seanet_cpu import _SConv1d

SMALL_KW = dict(n_filters=16, ratios=(5, 2), dimension=32)


def _latents(B, dim, frames, seed):
    return 3.0 * torch.randn(B, dim, frames, generator=torch.Generator().manual_seed(2000 + seed))


# ------------------------------------------------------------------------------------ the restatement
class _SConvTranspose1d(nn.Module):
    """EnCodec's non-causal SConvTranspose1d from nn.ConvTranspose1d + torch.nn.utils.parametrizations.weight_norm (default dim 0)"""

    def __init__(self, ci, co, k, stride):
        super().__init__()
        self.convtr = torch.nn.utils.parametrizations.weight_norm(nn.ConvTranspose1d(ci, co, k, stride=stride))
        self.k, self.stride = k, stride

    def load(self, sd, prefix):
        g = self.convtr.parametrizations.weight.original0
        assert tuple(g.shape) == tuple(sd[f"{prefix}.convtr.convtr.weight_g"].shape) == (self.convtr.in_channels, 1, 1)
        g.data.copy_(sd[f"{prefix}.convtr.convtr.weight_g"])
        self.convtr.parametrizations.weight.original1.data.copy_(sd[f"{prefix}.convtr.convtr.weight_v"])
        self.convtr.bias.data.copy_(sd[f"{prefix}.convtr.convtr.bias"])

    def forward(self, x):
        y = self.convtr(x)
        total = self.k - self.stride
        right = total // 2
        left = total - right
        return y[..., left:y.shape[-1] - right]  # encodec's unpad1d


class _Independent(nn.Module):
    def __init__(self, cfg, sd):
        super().__init__()
        mods = []
        for e in D.layout(cfg):
            i, kind = e[0], e[1]
            if kind == "elu":
                mods.append(nn.ELU())
            elif kind == "conv":
                m = _SConv1d(e[2], e[3], e[4])
                m.load(sd, f"model.{i}")
                mods.append(m)
            elif kind == "convtr":
                m = _SConvTranspose1d(e[2], e[3], e[4], e[5])
                m.load(sd, f"model.{i}")
                mods.append(m)
            elif kind == "res":
                a, b, sc = _SConv1d(e[2], e[3], e[4], dilation=e[5]), _SConv1d(e[3], e[2], 1), _SConv1d(e[2], e[2], 1)
                a.load(sd, f"model.{i}.block.1"), b.load(sd, f"model.{i}.block.3"), sc.load(sd, f"model.{i}.shortcut")
                mods.append(nn.ModuleDict(dict(block=nn.Sequential(nn.ELU(), a, nn.ELU(), b), shortcut=sc)))
            else:
                l = nn.LSTM(e[2], e[2], e[3])
                l.load_state_dict({k.split(".lstm.")[1]: v for k, v in sd.items() if k.startswith(f"model.{i}.lstm.")})
                mods.append(l)
        self.mods = nn.ModuleList(mods)

    def forward(self, z):
        x = z
        for m in self.mods:
            if isinstance(m, nn.ModuleDict):
                x = m["shortcut"](x) + m["block"](x)
            elif isinstance(m, nn.LSTM):
                t = x.permute(2, 0, 1)  # SLSTM: time first
                x = (m(t)[0] + t).permute(1, 2, 0)
            else:
                x = m(x)
        return x[:, 0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_module_construction(seed):
    for cfg in (D.config(), D.SMALL, D.config(n_filters=16, ratios=(3, 7), dimension=16, n_residual_layers=2, lstm=1)):
        sd = D.random_state(cfg, seed)
        net = _Independent(cfg, sd).double().eval()
        for frames in (1, 2, 11):
            z = _latents(2, cfg["dimension"], frames, seed).double()
            with torch.no_grad():
                want = net(z)
            got = D.decode(sd, cfg, z)
            assert got.shape == want.shape == (2, frames * D.hop(cfg))
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (seed, frames)


# ------------------------------------------------------------------------------------ state dicts and loaders
def test_state_dict_keys_and_shapes():
    import voicebox_pytorch_amd as vbx

    for cfg, kw in ((D.config(), {}), (D.SMALL, SMALL_KW), (D.config(n_residual_layers=2, lstm=1), dict(n_residual_layers=2, lstm=1)),
                    (D.config(lstm=0), dict(lstm=0))):
        dec = vbx.SEANetDecoder(**kw)
        got = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
        assert got == D.expected_shapes(cfg)
    dec = vbx.SEANetDecoder()
    sd = dec.state_dict()
    assert dec.hop_length == 320 and dec.hidden == 512
    assert tuple(sd["model.3.convtr.convtr.weight_v"].shape) == (512, 256, 16) and tuple(sd["model.3.convtr.convtr.weight_g"].shape) == (512, 1, 1)
    assert "model.1.lstm.weight_hh_l1" in sd and tuple(sd["model.15.conv.conv.weight_v"].shape) == (1, 32, 7) and "model.4.shortcut.conv.conv.bias" in sd
    plain = vbx.SEANetDecoder(norm="none").state_dict()
    assert "model.3.convtr.convtr.weight" in plain and not any(k.endswith("weight_g") for k in plain)


def _other_layouts(sd):
    par = {}
    for k, v in sd.items():
        k = k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1")
        par[k] = v
    whole = {"decoder." + k: v for k, v in sd.items()}
    whole["encoder.model.0.conv.conv.bias"] = torch.zeros(3)
    whole["quantizer.vq.layers.0._codebook.embed"] = torch.zeros(4, 128)
    return par, whole


def test_three_layouts_load_to_identical_folded_weights():
    import voicebox_pytorch_amd as vbx

    cfg = D.config()
    sd = D.random_state(cfg, 3)
    par, whole = _other_layouts(sd)
    decs = []
    for d in (sd, par, whole):
        m = vbx.SEANetDecoder()
        m.load_state_dict(d)
        decs.append(m)
    ref = decs[0].folded_weights()
    assert len(ref) == 1 + 4 * 4 + 1
    for m in decs[1:]:
        other = m.folded_weights()
        assert other.keys() == ref.keys() and all(torch.equal(other[k], ref[k]) for k in ref)
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), decs[0].state_dict().values()))
    for name, w in ref.items():  # and they are the fold of the restatement
        want = D.fold_tr(sd, name) if f"{name}.convtr.convtr.bias" in sd else S.fold(sd, name)
        assert torch.allclose(w.double(), want, rtol=1e-6, atol=0), name
    # the packed launch list exists without a GPU and is rebuilt on a version bump only
    ops = decs[0].packed_ops()
    assert ops is decs[0].packed_ops() and len(ops) == 1 + 1 + 3 * 4 + 1  # first convolution, LSTM, three launches a stage, last convolution
    assert [o["op"] for o in ops[:5]] == ["conv", "lstm", "convtr", "conv", "tail"] and ops[-1]["op"] == "conv_out"
    assert tuple(ops[2]["w"].shape) == (8 * 256, 1024) and ops[2]["w"].dtype == torch.float16 and tuple(ops[-1]["w"].shape) == (7, 32)
    with torch.no_grad():
        decs[0].model[3].convtr.convtr.bias.mul_(2)
    assert decs[0].packed_ops() is not ops


def test_from_checkpoint_recovers_the_configuration(tmp_path):
    import voicebox_pytorch_amd as vbx

    cfg = D.config(n_filters=16, ratios=(5, 3, 2), dimension=64, n_residual_layers=2, lstm=1, kernel_size=5, last_kernel_size=3)
    sd = D.random_state(cfg, 4)
    path = tmp_path / "dec.pt"
    torch.save({"state_dict": {"decoder." + k: v for k, v in sd.items()}}, path)
    dec = vbx.SEANetDecoder.from_checkpoint(str(path))
    assert (dec.n_filters, dec.ratios, dec.dimension, dec.n_residual_layers, dec.lstm, dec.kernel_size, dec.last_kernel_size, dec.norm) == \
        (16, (5, 3, 2), 64, 2, 1, 5, 3, "weight_norm")
    assert not dec.training and dec.hop_length == 30 and dec.hidden == 128
    assert all(torch.equal(dec.state_dict()[k], v) for k, v in sd.items())
    dec0 = vbx.SEANetDecoder.from_state_dict(D.random_state(D.config(lstm=0), 0))
    assert dec0.lstm == 0 and dec0.ratios == (8, 5, 4, 2)
    with pytest.raises(RuntimeError, match="SEANetDecoder"):
        vbx.SEANetDecoder.from_state_dict(S.random_state(S.config(), 0))  # an encoder is not a decoder


def test_from_encodec_checkpoint_without_a_vocoder_is_a_complete_codec(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = {"encoder." + k: v for k, v in S.random_state(dict(S.DEFAULT, **SMALL_KW), 5).items()}
    sd.update({"decoder." + k: v for k, v in D.random_state(D.SMALL, 6).items()})
    g = torch.Generator().manual_seed(0)
    for q in range(4):
        sd[f"quantizer.vq.layers.{q}._codebook.embed"] = torch.randn(64, 32, generator=g)
    path = tmp_path / "encodec.pt"
    torch.save(sd, path)
    codec = vbx.EncodecVocoCodec.from_encodec_checkpoint(str(path))
    assert isinstance(codec.encoder, vbx.SEANetEncoder) and isinstance(codec.vocoder, vbx.SEANetDecoder)
    assert codec.rvq.num_quantizers == 4 and codec.latent_dim == 32 and codec.downsample_factor == 10 == codec.vocoder.hop_length
    assert codec.vocoder.ratios == codec.encoder.ratios == (5, 2) and not codec.vocoder.training
    assert all(torch.equal(codec.vocoder.state_dict()[k], v) for k, v in D.random_state(D.SMALL, 6).items())
    voc = nn.Identity()  # a vocoder that is passed is used, and the decoder half is not read
    assert vbx.EncodecVocoCodec.from_encodec_checkpoint(str(path), vocoder=voc).vocoder is voc
    torch.save({k: v for k, v in sd.items() if not k.startswith("decoder.")}, path)
    with pytest.raises(KeyError, match="decoder"):
        vbx.EncodecVocoCodec.from_encodec_checkpoint(str(path))


# ------------------------------------------------------------------------------------ limits
@pytest.mark.parametrize("kw", [
    dict(causal=True), dict(pad_mode="constant"), dict(norm="layer_norm"), dict(norm="time_group_norm"), dict(activation="ReLU"),
    dict(activation_params={"alpha": 0.5}), dict(channels=2), dict(true_skip=True), dict(compress=4), dict(n_filters=24),
    dict(n_filters=80), dict(ratios=(8, 5, 4, 2, 2)), dict(ratios=()), dict(ratios=(9, 2)), dict(ratios=(4, 1)),
    dict(n_residual_layers=0), dict(n_residual_layers=4), dict(dilation_base=3), dict(lstm=3), dict(lstm=-1), dict(dimension=100),
    dict(dimension=520), dict(kernel_size=6), dict(kernel_size=9), dict(last_kernel_size=4), dict(last_kernel_size=9),
    dict(residual_kernel_size=5), dict(final_activation="Tanh"), dict(trim_right_ratio=0.5)])
def test_constructor_limits_raise(kw):
    import voicebox_pytorch_amd as vbx

    with pytest.raises(NotImplementedError, match="SEANetDecoder"):
        vbx.SEANetDecoder(**kw)


@pytest.mark.parametrize("kw", [
    dict(n_filters=64, ratios=(8, 8, 8, 8), dimension=512, n_residual_layers=3),  # the widest: 1024 -> 512, k 16, stride 8; an LSTM of 1024
    dict(n_filters=64, ratios=(8, 5, 4, 2)), dict(n_filters=48, ratios=(2, 2, 2, 8)), dict(n_filters=64, ratios=(2, 2, 2, 5)),
    dict(n_filters=16, ratios=(2,), dimension=8, lstm=0, kernel_size=1, last_kernel_size=1),
    dict(n_filters=64, ratios=(8,), n_residual_layers=3, lstm=1)])
def test_corners_of_the_served_range_have_a_tile(kw):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    dec = vbx.SEANetDecoder(**kw)
    last = D.layout(D.config(**kw))[-1][0]
    for e in D.layout(D.config(**kw)):
        if e[1] == "convtr":
            assert _lib.call_value("vbx_seanet_convtr_tile", e[2], e[5]) in (16, 32, 64, 128), (kw, e)
        convs = [(e[2], 0, e[4], 1)] if e[1] == "conv" and e[0] != last else [(e[2], 0, e[4], e[5]), (e[3], e[2], 1, 1)] if e[1] == "res" else []
        for cin, c2, k, dil in convs:
            assert _lib.call_value("vbx_seanet_conv_tile", cin, c2, k, 1, dil) in (16, 32, 64, 128), (kw, e)
    assert dec.hidden % 32 == 0 and dec.hidden <= 1024 and len(dec.packed_ops()) >= 5
    assert _lib.call_value("vbx_seanet_convtr_tile", 512, 8) == 64 and _lib.call_value("vbx_seanet_convtr_tile", 1024, 8) == 32
    for C, r in ((1040, 8), (24, 2), (64, 1), (64, 9)):  # what a refusal looks like
        with pytest.raises(_lib.VbxError, match="vbx_seanet_convtr"):
            _lib.call_value("vbx_seanet_convtr_tile", C, r)


def test_cpu_forward_raises():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    dec = vbx.SEANetDecoder(**SMALL_KW)
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
        dec(torch.zeros(1, 32, 5))
    with pytest.raises(ValueError):
        dec(torch.zeros(1, 5, 32))  # frames-major latents: the channel axis is wrong
    with pytest.raises(ValueError):
        dec(torch.zeros(32, 5))


# ------------------------------------------------------------------------------------ the phase packing
@pytest.mark.parametrize("r", [2, 5, 8])
def test_packed_convtr_weight_reproduces_conv_transpose(r):
    """the module's own packed weight [r Co, 2C] times the operand rows [a_j | a_{j-1}], j = 0 .. L, laid out as the kernel lays them
    out (row j's r Co results from trimmed position j r - left on), is F.conv_transpose1d + the trim"""
    import voicebox_pytorch_amd as vbx

    C, Co = 32, 16
    g = torch.Generator().manual_seed(r)
    w = torch.randn(C, Co, 2 * r, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    wp = vbx.SEANetDecoder._convtr_weight(w, r)
    assert tuple(wp.shape) == (r * Co, 2 * C)
    left = r - r // 2
    for L in (1, 2, 7):
        a = torch.randn(2, C, L, generator=g, dtype=torch.float64)
        want = D.sconvtr(a, w, b, r).transpose(1, 2)  # [B, L r, Co]
        al = F.pad(a.transpose(1, 2), (0, 0, 1, 1))  # [B, L + 2, C]: a_{-1} = a_L = 0
        rows = torch.cat([al[:, 1:], al[:, :-1]], dim=2)  # row j = [a_j | a_{j-1}], j = 0 .. L
        full = (rows @ wp.t()).reshape(2, (L + 1) * r, Co) + b
        got = full[:, left:left + L * r]
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (r, L)


# ------------------------------------------------------------------------------------ the bound against planted faults
def test_bound_is_far_below_every_fault():
    """Every planted fault of the restatement moves max |delta| / RMS(output) by at least 10 x BOUND_B_SMALL, the GPU tests' bound of
    the small configuration against plain fp64: n_filters 16, ratios (5, 2) (an odd ratio: swap_trim is invisible for even ones),
    dimension 32; z = 3 randn(2, 32, frames), frames in {3, 11}, seeds 0 .. 2.  (The real configuration dilutes the faults.)"""
    from test_seanet_dec_gpu import BOUND_B_SMALL

    cfg = D.SMALL
    worst = {}
    for seed in (0, 1, 2):
        sd = D.random_state(cfg, seed)
        for frames in (3, 11):
            z = _latents(2, 32, frames, seed).double()
            ref = D.decode(sd, cfg, z)
            for fault in D.FAULTS:
                got = D.decode(sd, cfg, z, fault=fault)
                assert got.shape == ref.shape
                worst[fault] = min(worst.get(fault, float("inf")), D.rel_err(got, ref))
    print("smallest max|delta|/RMS per fault:", {k: f"{v:.3g}" for k, v in worst.items()}, "BOUND_B_SMALL", BOUND_B_SMALL)
    assert set(worst) == set(D.FAULTS)
    for fault, e in worst.items():
        assert e >= 10 * BOUND_B_SMALL, (fault, e, BOUND_B_SMALL)
