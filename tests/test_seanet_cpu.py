"""Host-side tests of voicebox_pytorch_amd.SEANetEncoder: the fp64 restatement tests/seanet_ref.py against an independent
construction from torch's own modules, the state-dict layouts and loaders, the constructor limits, and that every planted fault of
the restatement is far above the parity bound the GPU tests use.  Parity with the `encodec` library itself is UNPINNED."""
import math

import pytest
import torch
from torch import nn

import seanet_ref as S


def _wave(B, T, seed):
    return 0.3 * torch.randn(B, T, generator=torch.Generator().manual_seed(1000 + seed))


# ------------------------------------------------------------------------------------ the restatement
class _SConv1d(nn.Module):
    """EnCodec's non-causal SConv1d from nn.Conv1d + torch.nn.utils.parametrizations.weight_norm, padding written out again here"""

    def __init__(self, ci, co, k, stride=1, dilation=1):
        super().__init__()
        self.conv = torch.nn.utils.parametrizations.weight_norm(nn.Conv1d(ci, co, k, stride=stride, dilation=dilation))
        self.k, self.stride, self.dilation = k, stride, dilation

    def load(self, sd, prefix):
        self.conv.parametrizations.weight.original0.data.copy_(sd[f"{prefix}.conv.conv.weight_g"])
        self.conv.parametrizations.weight.original1.data.copy_(sd[f"{prefix}.conv.conv.weight_v"])
        self.conv.bias.data.copy_(sd[f"{prefix}.conv.conv.bias"])

    def forward(self, x):
        L = x.shape[-1]
        total = (self.k - 1) * self.dilation + 1 - self.stride
        n_frames = (L - ((self.k - 1) * self.dilation + 1) + total) / self.stride + 1  # encodec's get_extra_padding_for_conv1d
        extra = (math.ceil(n_frames) - 1) * self.stride + ((self.k - 1) * self.dilation + 1 - total) - L
        right = total // 2
        left, right = total - right, right + extra
        cut = 0
        if L <= max(left, right):
            cut = max(left, right) - L + 1
            x = nn.functional.pad(x, (0, cut))
        x = nn.functional.pad(x, (left, right), mode="reflect")
        return self.conv(x[..., :x.shape[-1] - cut])


class _Independent(nn.Module):
    def __init__(self, cfg, sd):
        super().__init__()
        mods = []
        for e in S.layout(cfg):
            i, kind = e[0], e[1]
            if kind == "elu":
                mods.append(nn.ELU())
            elif kind == "conv":
                m = _SConv1d(e[2], e[3], e[4], stride=e[5])
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

    def forward(self, wave):
        x = wave[:, None]
        for m in self.mods:
            if isinstance(m, nn.ModuleDict):
                x = m["shortcut"](x) + m["block"](x)
            elif isinstance(m, nn.LSTM):
                t = x.permute(2, 0, 1)  # SLSTM: time first
                x = (m(t)[0] + t).permute(1, 2, 0)
            else:
                x = m(x)
        return x.transpose(1, 2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_module_construction(seed):
    cfg = S.config()
    sd = S.random_state(cfg, seed)
    net = _Independent(cfg, sd).double().eval()
    for T in (5, 321, 640, 3237):
        wave = _wave(2, T, seed).double()
        with torch.no_grad():
            want = net(wave)
        got = S.encode(sd, cfg, wave)
        assert got.shape == want.shape == (2, S.frames(cfg, T), 128)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (seed, T)


def test_frames_follow_the_ceil_chain():
    cfg = S.config()
    assert [S.frames(cfg, T) for T in (3237, 640, 321, 5)] == [11, 2, 2, 1]
    sd = S.random_state(cfg, 0)
    for T in (5, 321, 640, 3237):
        assert S.encode(sd, cfg, _wave(1, T, 0)).shape == (1, S.frames(cfg, T), 128)
    import voicebox_pytorch_amd as vbx

    enc = vbx.SEANetEncoder()
    assert [enc.frames(T) for T in (3237, 640, 321, 5)] == [11, 2, 2, 1] and enc.hop_length == 320


def test_short_input_rule_in_the_deep_layers():
    """T = 5 runs pad1d's short-input rule in 6 of the 10 padded convolutions: the last three strided ones, the final one and the
    k 3 convolutions of the last two Resnet blocks (lengths 3, 1, 1, 1 and 1, 1); the earlier ones see 5 or 3 samples, more than
    their padding.  The 1 x 1 convolutions have no padding.  (test_restatement_equals_module_construction covers T = 5.)"""
    cfg = S.config()
    L, hits, padded = 5, [], 0
    for e in S.layout(cfg):
        if e[1] in ("conv", "res"):
            stride, dil = (e[5], 1) if e[1] == "conv" else (1, e[5])
            left, right, extra = S.conv_pads(L, e[4], stride, dil)
            padded += 1
            if L <= max(left, right + extra):
                hits.append((e[0], L))
            L = -(-L // stride)
    assert padded == 10 and hits == [(6, 3), (7, 1), (9, 1), (10, 1), (12, 1), (15, 1)] and L == 1  # (model index, input length)
    x = torch.arange(1.0, 4.0)[None, None]
    assert S.pad1d(x, 4, 5).tolist() == [[[0.0, 0.0, 3.0, 2.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0]]]


# ------------------------------------------------------------------------------------ state dicts and loaders
def test_state_dict_keys_and_shapes():
    import voicebox_pytorch_amd as vbx

    for cfg, kw in ((S.config(), {}), (S.SMALL, dict(n_filters=16, ratios=(4, 2), dimension=32)),
                    (S.config(n_residual_layers=2, lstm=1), dict(n_residual_layers=2, lstm=1))):
        enc = vbx.SEANetEncoder(**kw)
        got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
        assert got == S.expected_shapes(cfg)
    sd = vbx.SEANetEncoder().state_dict()
    assert "model.13.lstm.weight_hh_l1" in sd and "model.15.conv.conv.weight_g" in sd and "model.1.block.3.conv.conv.bias" in sd
    plain = vbx.SEANetEncoder(norm="none").state_dict()
    assert "model.0.conv.conv.weight" in plain and not any(k.endswith("weight_g") for k in plain)


def _other_layouts(sd):
    par = {}
    for k, v in sd.items():
        k = k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1")
        par[k] = v
    whole = {"encoder." + k: v for k, v in sd.items()}
    whole["decoder.model.0.conv.conv.bias"] = torch.zeros(3)
    whole["quantizer.vq.layers.0._codebook.embed"] = torch.zeros(4, 128)
    return par, whole


def test_three_layouts_load_to_identical_folded_weights():
    import voicebox_pytorch_amd as vbx

    cfg = S.config()
    sd = S.random_state(cfg, 3)
    par, whole = _other_layouts(sd)
    encs = []
    for d in (sd, par, whole):
        e = vbx.SEANetEncoder()
        e.load_state_dict(d)
        encs.append(e)
    ref = encs[0].folded_weights()
    assert len(ref) == 1 + 4 * 4 + 1
    for e in encs[1:]:
        other = e.folded_weights()
        assert other.keys() == ref.keys() and all(torch.equal(other[k], ref[k]) for k in ref)
        assert all(torch.equal(a, b) for a, b in zip(e.state_dict().values(), encs[0].state_dict().values()))
    for name, w in ref.items():  # and they are the fold of the restatement
        assert torch.allclose(w.double(), S.fold(sd, name), rtol=1e-6, atol=0), name
    # the packed launch list exists without a GPU and is rebuilt on a version bump only
    ops = encs[0].packed_ops()
    assert ops is encs[0].packed_ops() and len(ops) == 1 + 3 * 4 + 1 + 1  # conv0, three launches a stage, the LSTM, the final convolution
    with torch.no_grad():
        encs[0].model[0].conv.conv.bias.mul_(2)
    assert encs[0].packed_ops() is not ops


def test_from_checkpoint_recovers_the_configuration(tmp_path):
    import voicebox_pytorch_amd as vbx

    cfg = S.config(n_filters=16, ratios=(5, 3, 2), dimension=64, n_residual_layers=2, lstm=1, kernel_size=5, last_kernel_size=3)
    sd = S.random_state(cfg, 4)
    path = tmp_path / "enc.pt"
    torch.save({"state_dict": {"encoder." + k: v for k, v in sd.items()}}, path)
    enc = vbx.SEANetEncoder.from_checkpoint(str(path))
    assert (enc.n_filters, enc.ratios, enc.dimension, enc.n_residual_layers, enc.lstm, enc.kernel_size, enc.last_kernel_size) == \
        (16, (5, 3, 2), 64, 2, 1, 5, 3)
    assert not enc.training and enc.hop_length == 30 and enc.hidden == 128
    assert all(torch.equal(enc.state_dict()[k], v) for k, v in sd.items())
    enc0 = vbx.SEANetEncoder.from_state_dict(S.random_state(S.config(lstm=0), 0))
    assert enc0.lstm == 0 and enc0.ratios == (8, 5, 4, 2)


def test_from_encodec_checkpoint_builds_the_codec(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = {"encoder." + k: v for k, v in S.random_state(S.config(), 5).items()}
    g = torch.Generator().manual_seed(0)
    for q in range(6):
        sd[f"quantizer.vq.layers.{q}._codebook.embed"] = torch.randn(64, 128, generator=g)
        sd[f"quantizer.vq.layers.{q}._codebook.cluster_size"] = torch.ones(64)
    sd["decoder.model.0.conv.conv.bias"] = torch.zeros(512)
    path = tmp_path / "encodec.pt"
    torch.save(sd, path)
    voc = nn.Identity()
    for bw, want in ((0, 2), (1, 4), (2, 6), (3, 6)):
        codec = vbx.EncodecVocoCodec.from_encodec_checkpoint(str(path), vocoder=voc, bandwidth_id=bw)
        assert codec.rvq.num_quantizers == want and codec.rvq.codebook_size == 64 and codec.latent_dim == 128
        assert codec.downsample_factor == 320 and isinstance(codec.encoder, vbx.SEANetEncoder) and codec.vocoder is voc
    books = codec.rvq.state_dict()["codebooks"]
    assert books.shape == (6, 64, 128) and torch.equal(books[3], sd["quantizer.vq.layers.3._codebook.embed"])
    with pytest.raises(ValueError, match="bandwidth_id"):
        vbx.EncodecVocoCodec.from_encodec_checkpoint(str(path), vocoder=voc, bandwidth_id=4)


# ------------------------------------------------------------------------------------ limits and untouched behaviour
@pytest.mark.parametrize("kw", [
    dict(causal=True), dict(pad_mode="constant"), dict(norm="layer_norm"), dict(norm="time_group_norm"), dict(activation="ReLU"),
    dict(activation_params={"alpha": 0.5}), dict(channels=2), dict(true_skip=True), dict(compress=4), dict(n_filters=24),
    dict(n_filters=80), dict(ratios=(8, 5, 4, 2, 2)), dict(ratios=()), dict(ratios=(9, 2)), dict(ratios=(4, 1)),
    dict(n_residual_layers=0), dict(n_residual_layers=4), dict(dilation_base=3), dict(lstm=3), dict(lstm=-1), dict(dimension=100),
    dict(dimension=520), dict(kernel_size=6), dict(kernel_size=9), dict(last_kernel_size=4), dict(last_kernel_size=9),
    dict(residual_kernel_size=5)])
def test_constructor_limits_raise(kw):
    import voicebox_pytorch_amd as vbx

    with pytest.raises(NotImplementedError, match="SEANetEncoder"):
        vbx.SEANetEncoder(**kw)


@pytest.mark.parametrize("kw", [
    dict(n_filters=64, ratios=(8, 8, 8, 8), dimension=512, n_residual_layers=3),  # the widest: 512 -> 1024, k 16, s 8; an LSTM of 1024
    dict(n_filters=64, ratios=(8, 5, 4, 2)), dict(n_filters=48, ratios=(8, 2, 2, 2)), dict(n_filters=64, ratios=(2, 2, 2, 5)),
    dict(n_filters=16, ratios=(2,), dimension=8, lstm=0, kernel_size=1, last_kernel_size=1),
    dict(n_filters=64, ratios=(8,), n_residual_layers=3, lstm=1)])
def test_corners_of_the_served_range_have_a_tile(kw):
    """every convolution of a configuration the constructor accepts has a tile in the convolution kernel (the constructor asks the
    library; here the answer is checked again, layer by layer) and packs into launchable operands"""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    enc = vbx.SEANetEncoder(**kw)
    for e in S.layout(S.config(**kw)):
        convs = [(e[2], e[4], e[5], 1)] if e[1] == "conv" and e[0] else [(e[2], e[4], 1, e[5]), (e[3], 1, 1, 1)] if e[1] == "res" else []
        for cin, k, stride, dil in convs:
            assert _lib.call_value("vbx_seanet_conv_tile", cin, e[2] if k == 1 and e[1] == "res" else 0, k, stride, dil) in (16, 32, 64, 128), (kw, e)
    assert enc.hidden % 32 == 0 and enc.hidden <= 1024 and len(enc.packed_ops()) >= 5
    with pytest.raises(_lib.VbxError, match="do not fit"):  # what a refusal looks like: beyond every accepted width
        _lib.call_value("vbx_seanet_conv_tile", 1024, 0, 16, 8, 1)


def test_cpu_forward_raises_and_codec_without_encoder_still_raises():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    enc = vbx.SEANetEncoder(n_filters=16, ratios=(4, 2), dimension=32)
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
        enc(torch.zeros(1, 100))
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 2, 100))
    codec = vbx.EncodecVocoCodec(rvq=vbx.ResidualVQ(dim=32, codebook_size=16, num_quantizers=2), vocoder=nn.Identity())
    with pytest.raises(NotImplementedError, match="SEANet"):
        codec.encode(torch.zeros(1, 100))


# ------------------------------------------------------------------------------------ the bound against planted faults
def test_bound_is_far_below_every_fault():
    """Every planted fault of the restatement moves max |delta| / RMS(output) by at least 10 x BOUND_B, the GPU tests' bound against
    plain fp64: real configuration, B = 2, T in {321, 3237}, seeds 0 .. 2.  (T = 5 is left out on purpose: its single frame
    dilutes the dropped ELU.)"""
    from test_seanet_gpu import BOUND_B

    cfg = S.config()
    worst = {}
    for seed in (0, 1, 2):
        sd = S.random_state(cfg, seed)
        for T in (321, 3237):
            wave = _wave(2, T, seed).double()
            ref = S.encode(sd, cfg, wave)
            for fault in S.FAULTS:
                got = S.encode(sd, cfg, wave, fault=fault)
                assert got.shape == ref.shape
                e = S.rel_err(got, ref)
                worst[fault] = min(worst.get(fault, float("inf")), e)
    print("smallest max|delta|/RMS per fault:", {k: f"{v:.3g}" for k, v in worst.items()}, "BOUND_B", BOUND_B)
    assert set(worst) == set(S.FAULTS)
    for fault, e in worst.items():
        assert e >= 10 * BOUND_B, (fault, e, BOUND_B)
