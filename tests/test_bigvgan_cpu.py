"""CPU (-m "not gpu"): voicebox_pytorch_amd.BigVGANGenerator's host side and its yardstick tests/bigvgan_ref.py.

 * the restatement equals, to 1e-12, an independent construction from nn.Conv1d / nn.ConvTranspose1d under
   torch.nn.utils.parametrizations.weight_norm with Activation1d written out afresh in the published forward's order;
 * the closed form of Activation1d (both replicate paddings as clamps) equals the padded construction at L = 1, 2, 5, 6, 7, 13;
 * the filter formula: sum 1, symmetric, Kaiser beta 4.6638, middle taps 0.4432 / 0.1286;
 * every state-dict layout loads to the same folded weights, strict=True; the loaders round-trip synthetic LOCAL files, REQUIRE config
   and raise ValueError where it contradicts the file;
 * every constructor refusal raises;
 * PLANTED FAULTS: each of bigvgan_tol.NETWORK_FAULTS moves the fp64 output far above the parity tolerance, which is DEFINED as one tenth
   of the smallest movement; the two faults a whole-network test cannot tell from rounding are held against the activation's
   per-element bound instead;
 * that bound (include/vbx.h, bigvgan_ref.act_bound) is not vacuous: an fp32 emulation of the documented order of operations stays
   inside it, the same emulation with u rounded to fp16 before the snake violates it.
Parity with the BigVGAN library itself is UNPINNED."""
import json

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bigvgan_ref as R
import bigvgan_tol as T


# ------------------------------------------------------------------------------------ the restatement against torch's own modules
class _LowPass(nn.Module):
    def __init__(self, stride):
        super().__init__()
        self.stride = stride
        self.register_buffer("filter", torch.zeros(1, 1, 12))

    def forward(self, x):  # kernel 12 (even): pad_left 5, pad_right 6
        C = x.shape[1]
        return F.conv1d(F.pad(x, (5, 6), mode="replicate"), self.filter.expand(C, -1, -1), stride=self.stride, groups=C)


class _Up(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", torch.zeros(1, 1, 12))

    def forward(self, x):  # ratio 2, kernel 12: pad 12 / 2 - 1 = 5, pad_left = 5 * 2 + (12 - 2) / 2 = 15, pad_right = 15
        C = x.shape[1]
        x = F.pad(x, (5, 5), mode="replicate")
        x = 2 * F.conv_transpose1d(x, self.filter.expand(C, -1, -1), stride=2, groups=C)
        return x[..., 15:-15]


class _Down(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = _LowPass(2)

    def forward(self, x):
        return self.lowpass(x)


class _SnakeAct(nn.Module):
    def __init__(self, ch, beta, logscale):
        super().__init__()
        self.logscale = logscale
        self.alpha = nn.Parameter(torch.zeros(ch))
        if beta:
            self.beta = nn.Parameter(torch.zeros(ch))

    def forward(self, x):
        alpha = self.alpha[None, :, None]
        beta = self.beta[None, :, None] if hasattr(self, "beta") else alpha
        if self.logscale:
            alpha, beta = torch.exp(alpha), torch.exp(beta)
        return x + (1.0 / (beta + 1e-9)) * torch.pow(torch.sin(x * alpha), 2)


class _Act1d(nn.Module):
    def __init__(self, ch, cfg):
        super().__init__()
        self.act, self.upsample, self.downsample = _SnakeAct(ch, cfg["activation"] == "snakebeta", cfg["snake_logscale"]), _Up(), _Down()

    def forward(self, x):
        return self.downsample(self.act(self.upsample(x)))


class _AMP(nn.Module):
    def __init__(self, ch, k, ds, cfg):
        super().__init__()
        wn = nn.utils.parametrizations.weight_norm
        first = nn.ModuleList([wn(nn.Conv1d(ch, ch, k, dilation=d, padding=(k * d - d) // 2)) for d in ds])
        if cfg["resblock"] == "1":
            self.convs1 = first
            self.convs2 = nn.ModuleList([wn(nn.Conv1d(ch, ch, k, padding=(k - 1) // 2)) for _ in ds])
            self.activations = nn.ModuleList([_Act1d(ch, cfg) for _ in range(2 * len(ds))])
        else:
            self.convs = first
            self.activations = nn.ModuleList([_Act1d(ch, cfg) for _ in ds])

    def forward(self, x):
        if hasattr(self, "convs1"):
            for c1, c2, a1, a2 in zip(self.convs1, self.convs2, self.activations[::2], self.activations[1::2]):
                x = c2(a2(c1(a1(x)))) + x
        else:
            for c, a in zip(self.convs, self.activations):
                x = c(a(x)) + x
        return x


class _Published(nn.Module):
    """BigVGAN as published, from torch's modules (fp64); its state dict has the published keys"""

    def __init__(self, cfg):
        super().__init__()
        wn = nn.utils.parametrizations.weight_norm
        self.cfg, c = cfg, cfg["upsample_initial_channel"]
        self.conv_pre = wn(nn.Conv1d(cfg["n_mels"], c, 7, padding=3))
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
            self.ups.append(nn.ModuleList([wn(nn.ConvTranspose1d(c, c // 2, k, u, padding=(k - u) // 2))]))
            c //= 2
            for rk, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
                self.resblocks.append(_AMP(c, rk, ds, cfg))
        self.activation_post = _Act1d(c, cfg)
        self.conv_post = wn(nn.Conv1d(c, 1, 7, padding=3, bias=cfg["use_bias_at_final"]))

    def forward(self, x):
        nk = len(self.cfg["resblock_kernel_sizes"])
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            for layer in up:
                x = layer(x)
            xs = None
            for j in range(nk):
                h = self.resblocks[i * nk + j](x)
                xs = h if xs is None else xs + h
            x = xs / nk
        x = self.conv_post(self.activation_post(x))
        return (torch.tanh(x) if self.cfg["use_tanh_at_final"] else torch.clamp(x, min=-1.0, max=1.0))[:, 0]


def _published(cfg, sd):
    new = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v.double()
           for k, v in sd.items()}
    pub = _Published(cfg).double()
    pub.load_state_dict(new, strict=True)
    return pub


@pytest.mark.parametrize("name", ["SMALL", "SMALL2"])
def test_restatement_equals_the_published_construction(name):
    cfg = getattr(R, name)
    sd = R.random_state(cfg, 0)
    mel = R.mels(2, cfg["n_mels"], 17, 1)
    ref = R.generate(sd, cfg, mel)
    with torch.no_grad():
        pub = _published(cfg, sd)(mel.double())
    assert ref.shape == pub.shape == (2, 17 * R.hop(cfg))
    assert float((ref - pub).abs().max()) <= 1e-12
    rms = float(ref.pow(2).mean().sqrt())
    assert 0.3 <= rms <= 0.9, rms
    pre = R.generate(sd, cfg, mel, final="none")
    assert float(pre.abs().max()) > 1.5  # the final function works on inputs that reach beyond +-1
    if name == "SMALL":  # input_log: the log of the clamped amplitudes in front
        amp = R.mels(2, cfg["n_mels"], 17, 2, amplitude=True)
        with torch.no_grad():
            pub = _published(cfg, sd)(torch.log(torch.clamp(amp.double(), min=1e-5)))
        assert float((R.generate(sd, cfg, amp, input_log=True) - pub).abs().max()) <= 1e-12


def test_wide_is_the_large_published_shape():
    assert R.hop(R.WIDE) == 256 and R.WIDE["upsample_initial_channel"] // 2 ** 6 == 24
    shapes = R.expected_shapes(R.WIDE)
    assert "conv_post.bias" not in shapes and shapes["conv_post.weight_v"] == (1, 24, 7) and shapes["ups.0.0.weight_g"] == (1536, 1, 1)


# ------------------------------------------------------------------------------------ Activation1d and its filters
def _act_inputs(C, L, seed, dtype=torch.float64, alpha_hi=4.0):
    g = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn(2, C, L, generator=g, dtype=dtype)
    alpha = 1.0 + (alpha_hi - 1.0) * torch.rand(C, generator=g, dtype=dtype)
    inv_beta = 1.0 / (1.0 + 2.0 * torch.rand(C, generator=g, dtype=dtype))
    return x, alpha, inv_beta


@pytest.mark.parametrize("L", [1, 2, 5, 6, 7, 13])
def test_closed_form_of_the_activation(L):
    """u[m] = 2 sum_i f_u[m + 5 - 2 i] x[clamp(i, 0, L - 1)], y[t] = sum_tau f_d[tau] s[clamp(2 t + tau - 5, 0, 2 L - 1)]: the two clamps
    act on different signals"""
    x, alpha, inv_beta = _act_inputs(3, L, L)
    g = torch.Generator().manual_seed(100 + L)
    f = R.kaiser_sinc_filter(torch.float64)
    for f_u, f_d in ((f, f), (torch.randn(12, generator=g, dtype=torch.float64), torch.randn(12, generator=g, dtype=torch.float64))):
        a, b = R.activation1d(x, alpha, inv_beta, f_u, f_d), R.activation1d_closed(x, alpha, inv_beta, f_u, f_d)
        assert a.shape == b.shape == x.shape
        assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(a.abs().max()))
    with torch.no_grad():  # and the module form of the independent construction
        m = _Act1d(3, dict(activation="snakebeta", snake_logscale=True)).double()
        m.act.alpha.copy_(torch.log(alpha)), m.act.beta.copy_(torch.log(1.0 / inv_beta))
        m.upsample.filter.copy_(f.reshape(1, 1, 12)), m.downsample.lowpass.filter.copy_(f.reshape(1, 1, 12))
        assert float((m(x) - R.activation1d_closed(x, alpha, 1.0 / (1.0 / inv_beta + 1e-9), f, f)).abs().max()) <= 1e-12


def test_filter_formula():
    from voicebox_pytorch_amd.bigvgan import kaiser_sinc_filter1d

    assert abs(R.kaiser_beta() - 4.6638) < 1e-4
    f64 = R.kaiser_sinc_filter(torch.float64)
    assert abs(float(f64.sum()) - 1.0) < 1e-15 and float((f64 - f64.flip(0)).abs().max()) < 1e-16
    assert abs(float(f64[5]) - 0.4432) < 5e-5 and abs(float(f64[4]) - 0.1286) < 5e-5
    f = kaiser_sinc_filter1d()  # what a freshly constructed module is filled with
    assert f.shape == (1, 1, 12) and f.dtype == torch.float32
    assert float((f.reshape(12).double() - f64).abs().max()) < 1e-7
    assert torch.equal(f.reshape(12), R.kaiser_sinc_filter(torch.float32))


# ------------------------------------------------------------------------------------ the activation's bound is not vacuous
def test_activation_bound_holds_for_the_documented_order_and_not_for_a_rounded_u():
    f = R.kaiser_sinc_filter(torch.float32)
    worst, broken = 0.0, 0.0
    for C, L, seed in ((8, 1, 0), (8, 2, 1), (8, 7, 2), (24, 65, 3)):
        x, alpha, inv_beta = _act_inputs(C, L, seed, torch.float32, alpha_hi=16.0)  # |alpha u| up to about 50
        x = x.half().float()
        ref, bound = R.act_bound(x.double(), alpha, inv_beta, f, f)
        worst = max(worst, float(((R.act_emulated(x, alpha, inv_beta, f, f).double() - ref).abs() / bound).max()))
        broken = max(broken, float(((R.act_emulated(x, alpha, inv_beta, f, f, round_u=True).double() - ref).abs() / bound).max()))
    print(f"vbx_bigvgan_act's order of operations in fp32 on the host: max |err| / bound {worst:.3f}; with u rounded to fp16: {broken:.1f}")
    assert worst <= 1.0
    assert broken > 3.0


@pytest.mark.parametrize("fault", T.KERNEL_ONLY_FAULTS)
def test_padding_faults_violate_the_activation_bound(fault):
    """the two faults the whole-network tolerance cannot see (bigvgan_tol.py): against the bound vbx_bigvgan_act is held to"""
    f = R.kaiser_sinc_filter(torch.float32)
    for L in (1, 2, 7, 65):
        x, alpha, inv_beta = _act_inputs(8, L, L, torch.float32)
        x = x.half().float()
        ref, bound = R.act_bound(x.double(), alpha, inv_beta, f, f)
        bad = R.activation1d(x.double(), alpha.double(), inv_beta.double(), f.double(), f.double(), fault=fault)
        ratio = (bad - ref).abs() / bound
        # both ends of every row: far outside in some channel (one whose sample there happens to be near zero moves little)
        assert float(ratio[..., 0].max(dim=1).values.min()) > 100 and float(ratio[..., -1].max(dim=1).values.min()) > 100, (fault, L)
        if L > 16:
            assert float(ratio[..., 8:-8].max()) < 1e-6  # and nothing in between: why the network dilutes them


# ------------------------------------------------------------------------------------ planted faults and the tolerance
def test_planted_faults_move_the_output_and_set_the_tolerance():
    tol, moves, emu = T.parity_tolerance()
    worst_emu = max(emu.values())
    lines = [f"tolerance (one tenth of the smallest whole-network planted fault's movement, max |delta| / RMS, fp64): {tol:.4e}"]
    for (name, fault), v in sorted(moves.items(), key=lambda kv: kv[1]):
        where = "single-kernel tests only" if fault in T.KERNEL_ONLY_FAULTS else "whole network"
        lines.append(f"  fault {fault:<14} config {name:<6} moves the output by {v:.4e}  ({where})")
    for name, v in emu.items():
        lines.append(f"  emulated-precision restatement vs fp64, config {name:<6}: {v:.4e} ({tol / v:.1f} x inside the tolerance)")
    print("\n".join(lines))
    T.write_section("cpu", lines)
    assert {f for _, f in moves} == set(R.FAULTS)  # every fault was planted somewhere
    net = {k: v for k, v in moves.items() if k[1] in T.NETWORK_FAULTS}
    assert all(v >= 10 * tol * (1 - 1e-12) for v in net.values())
    # a whole-network fault must stand 20 times above what the contract's roundings alone cost ...
    assert all(v >= 20 * worst_emu for v in net.values()), (net, worst_emu)
    # ... and the faults taken out of the list are exactly those that do not
    for fault in T.KERNEL_ONLY_FAULTS:
        assert min(v for (_, f), v in moves.items() if f == fault) < 20 * worst_emu, fault
    # the roundings must leave room for the kernels' fp32 summation order: at most half the tolerance
    assert all(v <= tol / 2 for v in emu.values()), (emu, tol)


# ------------------------------------------------------------------------------------ state dicts and files
def _config_json(cfg, **over):
    out = dict(num_mels=cfg["n_mels"], upsample_initial_channel=cfg["upsample_initial_channel"], upsample_rates=list(cfg["upsample_rates"]),
               upsample_kernel_sizes=list(cfg["upsample_kernel_sizes"]), resblock=cfg["resblock"],
               resblock_kernel_sizes=list(cfg["resblock_kernel_sizes"]), resblock_dilation_sizes=[list(d) for d in cfg["resblock_dilation_sizes"]],
               activation=cfg["activation"], snake_logscale=cfg["snake_logscale"], use_tanh_at_final=cfg["use_tanh_at_final"],
               use_bias_at_final=cfg["use_bias_at_final"], sampling_rate=24000, segment_size=8192)
    out.update(over)
    return out


def _generator(cfg, **kw):
    import voicebox_pytorch_amd as vbx

    return vbx.BigVGANGenerator(**cfg, **kw)


def _same_folded(gen, sd, cfg, exact=False):
    got = gen.folded_weights()
    assert set(got) == {p for p, *_ in R.layout(cfg)}
    for p, w in got.items():
        ref = R.fold(sd, p, torch.float32)
        assert w.shape == ref.shape
        assert torch.equal(w, ref) if exact else float((w - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), p
    for p, _ in R.act_layout(cfg):
        mod = gen.get_submodule(p)
        assert torch.equal(mod.act.alpha, sd[f"{p}.act.alpha"]) and torch.equal(mod.upsample.filter, sd[f"{p}.upsample.filter"])


@pytest.mark.parametrize("name", ["SMALL", "SMALL2"])
def test_state_dict_layouts(name):
    cfg = getattr(R, name)
    sd = R.random_state(cfg, 1, calibrate=False)
    gen = _generator(cfg)
    assert {k: tuple(v.shape) for k, v in gen.state_dict().items()} == R.expected_shapes(cfg)
    assert gen.hop_length == R.hop(cfg)
    assert gen.load_state_dict(sd, strict=True) is not None
    _same_folded(gen, sd, cfg)
    back = gen.state_dict()  # a strict round trip
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    new = {}
    for k, v in sd.items():
        new[k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1")] = v
    gen2 = _generator(cfg)
    gen2.load_state_dict(new, strict=True)
    _same_folded(gen2, sd, cfg)
    gen3 = _generator(cfg)
    gen3.load_state_dict({"generator": sd}, strict=True)
    _same_folded(gen3, sd, cfg)
    plain = {k: v for k, v in sd.items() if "weight_" not in k}
    for p, *_ in R.layout(cfg):
        plain[f"{p}.weight"] = R.fold(sd, p, torch.float32)
    gen4 = _generator(cfg)
    gen4.load_state_dict(plain, strict=True)
    _same_folded(gen4, plain, cfg, exact=True)
    assert set(gen4.state_dict()) == set(plain)
    gen4.load_state_dict(sd, strict=True)  # and back under weight norm
    assert set(gen4.state_dict()) == set(sd)
    with pytest.raises(RuntimeError):
        _generator(cfg).load_state_dict({k: v for k, v in sd.items() if not k.startswith("activation_post")})
    with pytest.raises(ValueError, match="filter"):  # a filter of another length
        _generator(cfg).load_state_dict(dict(sd, **{"activation_post.upsample.filter": torch.zeros(1, 1, 6)}))
    # the loaded buffers are the ones in use, not the formula's
    other = dict(sd, **{"activation_post.downsample.lowpass.filter": torch.full((1, 1, 12), 1.0 / 12)})
    gen5 = _generator(cfg)
    gen5.load_state_dict(other)
    assert torch.equal(gen5.activation_post.downsample.lowpass.filter, other["activation_post.downsample.lowpass.filter"])


@pytest.mark.parametrize("name", ["SMALL", "SMALL2"])
def test_loaders_round_trip_and_require_config(name, tmp_path):
    import voicebox_pytorch_amd as vbx

    cfg = getattr(R, name)
    sd = R.random_state(cfg, 2, calibrate=False)
    path = tmp_path / "bigvgan_generator.pt"
    torch.save({"generator": sd}, path)
    cj = _config_json(cfg)
    gen = vbx.BigVGANGenerator.from_checkpoint(str(path), config=cj, input_log=True)
    for key in ("n_mels", "upsample_initial_channel", "upsample_rates", "upsample_kernel_sizes", "resblock", "resblock_kernel_sizes",
                "resblock_dilation_sizes", "activation", "snake_logscale", "use_tanh_at_final", "use_bias_at_final"):
        assert getattr(gen, key) == cfg[key], key
    assert not gen.training and gen.input_log
    _same_folded(gen, sd, cfg)
    assert set(gen.state_dict()) == set(sd)
    cpath = tmp_path / "config.json"
    cpath.write_text(json.dumps(cj))
    gen = vbx.BigVGANGenerator.from_checkpoint(str(path), config=str(cpath))  # a LOCAL json file
    assert gen.resblock_dilation_sizes == cfg["resblock_dilation_sizes"] and not gen.input_log
    gen = vbx.BigVGANGenerator.from_state_dict(sd, cj)
    _same_folded(gen, sd, cfg)
    # without config: ValueError naming the three things no state dict can say
    for call in (lambda: vbx.BigVGANGenerator.from_checkpoint(str(path)), lambda: vbx.BigVGANGenerator.from_state_dict(sd)):
        with pytest.raises(ValueError) as e:
            call()
        assert all(word in str(e.value) for word in ("dilations", "snake_logscale", "use_tanh_at_final"))
    # a config that contradicts the file
    other_act = "snake" if cfg["activation"] == "snakebeta" else "snakebeta"
    bad = [("upsample_rates", [8, 2]), ("resblock", "2" if cfg["resblock"] == "1" else "1"), ("num_mels", 80),
           ("resblock_kernel_sizes", [3, 9, 11][:len(cfg["resblock_kernel_sizes"])]), ("upsample_initial_channel", 128),
           ("resblock_dilation_sizes", [[1], [1], [1]][:len(cfg["resblock_kernel_sizes"])]), ("activation", other_act),
           ("use_bias_at_final", not cfg["use_bias_at_final"])]
    for key, val in bad:
        with pytest.raises(ValueError):
            vbx.BigVGANGenerator.from_state_dict(sd, dict(cj, **{key: val}))
    for key in ("resblock_dilation_sizes", "activation"):
        with pytest.raises(ValueError):
            vbx.BigVGANGenerator.from_state_dict(sd, {k: v for k, v in cj.items() if k != key})
    # keys the file may omit take the library's defaults
    short = {k: v for k, v in cj.items() if k not in ("use_tanh_at_final", "use_bias_at_final", "snake_logscale")}
    if cfg["use_bias_at_final"]:
        gen = vbx.BigVGANGenerator.from_state_dict(sd, short)
        assert gen.use_tanh_at_final and gen.use_bias_at_final and not gen.snake_logscale
    else:  # the default says a bias, the file has none
        with pytest.raises(ValueError):
            vbx.BigVGANGenerator.from_state_dict(sd, short)
    with pytest.raises(RuntimeError):
        vbx.BigVGANGenerator.from_state_dict({"conv_pre.bias": torch.zeros(4)}, cj)


REFUSED = [dict(n_mels=0), dict(n_mels=513), dict(upsample_initial_channel=520), dict(upsample_initial_channel=2048),
           dict(upsample_initial_channel=64), dict(upsample_initial_channel=1664),
           dict(upsample_rates=(2,) * 7, upsample_kernel_sizes=(4,) * 7, upsample_initial_channel=1024),
           dict(upsample_rates=(), upsample_kernel_sizes=()), dict(upsample_rates=(5, 8, 2, 2), upsample_kernel_sizes=(10, 16, 4, 4)),
           dict(upsample_rates=(10, 8, 2, 2), upsample_kernel_sizes=(20, 16, 4, 4)), dict(upsample_kernel_sizes=(16, 15, 4, 4)),
           dict(upsample_kernel_sizes=(16, 16, 4, 8)), dict(resblock="3"), dict(resblock_kernel_sizes=(3, 7, 13)),
           dict(resblock_kernel_sizes=(3, 4, 11)), dict(resblock_kernel_sizes=(1, 7, 11)), dict(resblock_dilation_sizes=((1, 3, 13),) * 3),
           dict(resblock_dilation_sizes=((0, 3, 5),) * 3), dict(resblock_dilation_sizes=((1, 3, 5, 7),) * 3),
           dict(resblock_dilation_sizes=((),) * 3), dict(resblock_kernel_sizes=(3, 5, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 4),
           dict(resblock_kernel_sizes=(), resblock_dilation_sizes=()), dict(activation="relu"), dict(activation="leaky"),
           dict(up_ratio=4), dict(down_ratio=4), dict(up_kernel_size=8), dict(down_kernel_size=24)]


@pytest.mark.parametrize("kw", REFUSED, ids=[",".join(f"{k}={v}" for k, v in kw.items())[:60] for kw in REFUSED])
def test_constructor_refusals(kw):
    import voicebox_pytorch_amd as vbx

    with pytest.raises(NotImplementedError, match="BigVGANGenerator: .* is not built"):
        vbx.BigVGANGenerator(**kw)


def test_accepted_edges_and_cpu_tensors():
    import voicebox_pytorch_amd as vbx

    gen = vbx.BigVGANGenerator(**R.WIDE)  # 1536 -> 24 over six stages
    assert gen.hop_length == 256 and gen.conv_post.cin == 24 and gen.conv_post.bias is None and "conv_post.bias" not in gen.state_dict()
    assert {k: tuple(v.shape) for k, v in gen.state_dict().items()} == R.expected_shapes(R.WIDE)
    vbx.BigVGANGenerator(n_mels=100, upsample_initial_channel=1024, upsample_rates=(8,), upsample_kernel_sizes=(16,),
                         resblock_kernel_sizes=(11,), resblock_dilation_sizes=((12, 12, 12),))
    gen = vbx.BigVGANGenerator(n_mels=1, upsample_initial_channel=16, upsample_rates=(2,), upsample_kernel_sizes=(4,), resblock="2",
                               resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),), activation="snake", snake_logscale=False)
    assert gen.hop_length == 2 and float(gen.activation_post.act.alpha.detach().min()) == 1.0  # not logscale: ones
    assert float(_generator(R.SMALL).activation_post.act.alpha.detach().abs().max()) == 0.0  # logscale: zeros
    assert isinstance(gen, vbx.BigVGANGenerator) and hasattr(gen, "mark_weights_dirty") and hasattr(gen, "fuse_act_max_channels")
    with pytest.raises(ValueError):
        vbx.BigVGANGenerator(upsample_kernel_sizes=(16, 16, 4))
    with pytest.raises(vbx._lib.VbxError):
        gen(torch.zeros(1, 1, 4))
    with pytest.raises(ValueError):
        gen(torch.zeros(1, 2, 4))
