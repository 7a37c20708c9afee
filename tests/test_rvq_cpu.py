"""CPU side of the residual vector quantizer: the checker of tests/rvq_ref.py against faults it must catch and searches it must
pass, the fp32 restatement on every input of tests/test_rvq_gpu.py, and the host logic of ResidualVQ / EncodecVocoCodec /
VocosDecoder.from_checkpoint(bandwidth_id=...) (state dicts, argument limits, error paths)."""
import pytest
import torch

import rvq_ref as rr
import vocos_ref as vr


# ----------------------------------------------------------------------------- the contract and its checker
@pytest.mark.parametrize("name,M,D,K", rr.PLANTED, ids=[p[0] for p in rr.PLANTED])
def test_bound_sits_below_the_fault_it_is_meant_to_catch(name, M, D, K):
    """planted inputs: searches of fp32 class (plain fp32, hi/lo-split fp16 and bf16 with lo . lo dropped) never exceed the bound
    and return the fp64 argmin wherever the bound forces it; ONE rounding of the operands to fp16 does exceed it"""
    x, cb = rr.case_inputs(name)
    x = x[0]
    for mode in ("fp32", "fp16x3", "bf16x3"):
        res = rr.check_search(x, cb, rr.search(x, cb, mode)[0])
        print(f"{name} {mode}: {res}")
        assert res["violations"] == 0 and res["forced_wrong"] == 0 and res["forced"] == M, (mode, res)
    res = rr.check_search(x, cb, rr.search(x, cb, "fp16")[0])
    print(f"{name} single fp16: {res}")
    assert res["violations"] > 0 and res["forced_wrong"] == res["violations"] and res["worst"] > 1.0, res


def test_planted_gaps_are_the_planted_multiples():
    x, cb = rr.case_inputs("planted-32")
    d = rr.distances64(x[0].double(), cb[0].double())
    two = torch.topk(d, 2, dim=1, largest=False)
    bound = (32 + 2) * rr.U23 * (x[0].double().norm(dim=1) + cb[0].double().norm(dim=1).max()) ** 2
    ratio = (two.values[:, 1] - two.values[:, 0]) / bound
    assert float(ratio.min()) > 1.4 and float(ratio.max()) < 6.1
    assert bool((two.indices[:, 0] // 2 == two.indices[:, 1] // 2).all())  # best and second best are one planted pair
    assert 0.25 < float((two.indices[:, 0] % 2).float().mean()) < 0.75    # either sign


@pytest.mark.parametrize("name", [c[0] for c in rr.CASES] + ["ties", "exact"])
def test_fp32_restatement_meets_the_contract_on_every_gpu_input(name):
    if name == "ties":
        x, cb, _ = rr.tie_case()
    elif name == "exact":
        x, cb, _ = rr.exact_case()
    else:
        x, cb = rr.case_inputs(name)
    x = x.reshape(-1, x.shape[-1])
    codes, quant = rr.search(x, cb)
    res = rr.check_search(x, cb, codes)
    print(f"{name}: {res}")
    assert res["violations"] == 0 and res["forced_wrong"] == 0, res
    assert torch.equal(quant, rr.gather_sum(codes, cb))


def test_checker_catches_wrong_codes():
    x, cb = rr.case_inputs("tail")
    x = x.reshape(-1, 32)
    codes, _ = rr.search(x, cb)
    bad = codes.clone()
    bad[5, 2] = (bad[5, 2] + 1) % 64
    res = rr.check_search(x, cb, bad)
    assert res["violations"] >= 1 and res["worst"] > 100.0
    # a second-best code at stage 0 is a violation there, and the later stages are judged on ITS residual: no pile-up
    d = rr.distances64(x.double(), cb[0].double())
    second = torch.topk(d, 2, dim=1, largest=False).indices[:, 1]
    codes2, _ = rr.search(x - cb[0][second], cb[1:])
    res = rr.check_search(x, cb, torch.cat((second[:, None], codes2), dim=1))
    assert res["violations"] == x.shape[0], res


def test_tie_and_exact_cases_are_what_they_claim():
    x, cb, expect = rr.tie_case()
    codes, _ = rr.search(x[0], cb)
    assert bool((codes[:, 0][expect >= 0] == expect[expect >= 0]).all()) and bool((codes[:, 0][expect < 0] == 17).all())
    x, cb, k0 = rr.exact_case()
    codes, quant = rr.search(x[0], cb)
    assert torch.equal(codes[:, 0], k0) and bool((codes[:, 1] == 5).all())
    assert int(cb[1].double().pow(2).sum(1).argmin()) in (5, 20)


# ----------------------------------------------------------------------------- ResidualVQ: host logic
def test_rvq_state_dict_layouts():
    import voicebox_pytorch_amd as vbx

    g = torch.Generator().manual_seed(0)
    cb = torch.randn(3, 16, 8, generator=g)
    m = vbx.ResidualVQ(dim=8, codebook_size=16, num_quantizers=3)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"codebooks": (3, 16, 8)} and m.codebooks.dtype == torch.float32
    m.load_state_dict({"codebooks": cb})
    assert torch.equal(m.codebooks, cb)
    for wrap in (lambda t: t[None], lambda t: t):  # vector_quantize_pytorch: [1, K, D] (one codebook head) or [K, D]
        m2 = vbx.ResidualVQ(dim=8, codebook_size=16, num_quantizers=3)
        m2.load_state_dict({f"layers.{q}._codebook.embed": wrap(cb[q]).double() for q in range(3)})
        assert torch.equal(m2.codebooks, cb) and m2.codebooks.dtype == torch.float32
    m3 = vbx.ResidualVQ(dim=8, codebook_size=16, num_quantizers=2)
    m3.load_state_dict({"codebook_weights": cb.reshape(48, 8)})  # Vocos's flat table; the first two codebooks of three
    assert torch.equal(m3.codebooks, cb[:2])
    with pytest.raises(RuntimeError):
        vbx.ResidualVQ(dim=8, codebook_size=16, num_quantizers=4).load_state_dict({"codebook_weights": cb.reshape(48, 8)})
    with pytest.raises(RuntimeError):
        m.load_state_dict({"codebooks": cb[:, :, :4]})


def test_published_layouts_load_through_a_parent_module():
    """the layouts are rewritten in the per-module hook, so a codec's own load_state_dict takes them under `rvq.` too"""
    import voicebox_pytorch_amd as vbx

    g = torch.Generator().manual_seed(1)
    cb = torch.randn(2, 16, 32, generator=g)
    for layout in ({f"rvq.layers.{q}._codebook.embed": cb[q][None] for q in range(2)}, {"rvq.codebook_weights": cb.reshape(32, 32)},
                   {"rvq.codebooks": cb}):
        codec = vbx.EncodecVocoCodec(rvq=vbx.ResidualVQ(dim=32, codebook_size=16, num_quantizers=2), vocoder=small_vocoder(vbx))
        sd = {k: v for k, v in codec.state_dict().items() if not k.startswith("rvq.")}
        codec.load_state_dict({**sd, **layout}, strict=True)
        assert torch.equal(codec.rvq.codebooks, cb)
    with pytest.raises(RuntimeError):
        codec.load_state_dict({**sd, "rvq.codebook_weights": cb.reshape(64, 16)})


@pytest.mark.parametrize("bad", [dict(dim=12), dict(dim=0), dict(dim=264), dict(codebook_size=1), dict(codebook_size=4097),
                                 dict(num_quantizers=0), dict(num_quantizers=33)])
def test_rvq_limits_raise(bad):
    import voicebox_pytorch_amd as vbx

    with pytest.raises(NotImplementedError, match=next(iter(bad))):
        vbx.ResidualVQ(**{**dict(dim=8, codebook_size=16, num_quantizers=2), **bad})


def test_rvq_entry_points_refuse_the_same_limits_before_any_launch():
    from voicebox_pytorch_amd import _lib

    l = _lib.lib()
    p = 4096  # a placeholder pointer: the arguments are validated on the host first
    good = dict(B=1, N=4, D=8, K=16, Q=2)
    for bad, word in ((dict(D=12), "dim"), (dict(D=264), "dim"), (dict(K=1), "codebook_size"), (dict(K=4097), "codebook_size"),
                      (dict(Q=0), "num_quantizers"), (dict(Q=33), "num_quantizers"), (dict(N=0), "N >= 1")):
        a = {**good, **bad}
        assert l.vbx_rvq_encode(p, p, p, p, None, a["B"], a["N"], a["D"], a["K"], a["Q"], 0, None) != 0
        assert word.encode() in l.vbx_last_error()
        assert l.vbx_rvq_decode(p, p, p, a["B"], a["N"], a["D"], a["K"], a["Q"], 1, 1, None) != 0
        assert word.encode() in l.vbx_last_error()
    assert l.vbx_rvq_norms(p, p, 2, 16, 12, None) != 0 and b"dim" in l.vbx_last_error()
    assert l.vbx_rvq_encode(None, p, p, p, None, 1, 4, 8, 16, 2, 0, None) != 0 and b"null operand" in l.vbx_last_error()


def small_vocoder(vbx, channels=32):
    return vbx.VocosDecoder(input_channels=channels, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64)


def test_cpu_tensors_and_bad_arguments_raise():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    rvq = vbx.ResidualVQ(dim=32, codebook_size=16, num_quantizers=2)
    codec = vbx.EncodecVocoCodec(rvq=rvq, vocoder=small_vocoder(vbx))
    z, codes = torch.zeros(1, 4, 32), torch.zeros(1, 2, 4, dtype=torch.int64)
    for call in (lambda: rvq(z), lambda: rvq.encode(z), lambda: rvq.decode(codes.transpose(1, 2)), lambda: codec.decode_to_codes(z),
                 lambda: codec.codes_to_latents(codes), lambda: codec.codes_to_features(codes), lambda: codec.decode(z)):
        with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
            call()
    with pytest.raises(ValueError):
        rvq(torch.zeros(1, 4, 16))
    with pytest.raises(ValueError):
        rvq.decode(codes.int().transpose(1, 2))
    with pytest.raises(ValueError):
        codec.codes_to_latents(torch.zeros(1, 3, 4, dtype=torch.int64))  # more quantizers than the table holds
    with pytest.raises(NotImplementedError, match="SEANet"):
        codec.encode(torch.zeros(1, 640))
    with pytest.raises(TypeError):
        vbx.EncodecVocoCodec(rvq=torch.nn.Identity(), vocoder=small_vocoder(vbx))
    assert (codec.latent_dim, codec.sampling_rate, codec.downsample_factor) == (32, 24000, 320)
    assert set(codec.state_dict()) >= {"rvq.codebooks", "vocoder.backbone.embed.weight"}


def test_voicebox_accepts_the_codec():
    import voicebox_pytorch_amd as vbx

    codec = vbx.EncodecVocoCodec(rvq=vbx.ResidualVQ(dim=32, codebook_size=16, num_quantizers=2), vocoder=small_vocoder(vbx))
    vb = vbx.VoiceBox(dim=64, depth=2, heads=2, audio_enc_dec=codec, condition_on_text=False)
    assert vb.audio_enc_dec is codec and vb.proj_in.in_features == 32


# ----------------------------------------------------------------------------- checkpoints
def adanorm_state(seed, channels=32, rows=4):
    """a Vocos-EnCodec state dict: the plain one of vocos_ref.random_state with every backbone AdaLayerNorm as scale / shift
    embedding tables of `rows` ids (final_layer_norm is a plain LayerNorm in that variant), and the flat codebook table"""
    sd = vr.random_state(channels, 64, 192, 2, 256, seed)
    g = torch.Generator().manual_seed(seed + 50)
    out = {}
    for k, v in sd.items():
        if k.endswith(".norm.weight") or k.endswith(".norm.bias"):
            table = torch.stack([v * 0 + (1.0 if k.endswith("weight") else 0.0) + 0.3 * torch.randn(64, generator=g) for _ in range(rows)])
            out[k.replace(".norm.weight", ".norm.scale.weight").replace(".norm.bias", ".norm.shift.weight")] = table
        else:
            out[k] = v
    out["feature_extractor.codebook_weights"] = torch.randn(5 * 16, channels, generator=g)
    return out


def test_from_checkpoint_folds_one_bandwidth_id(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = adanorm_state(0)
    path = str(tmp_path / "vocos_encodec.pt")
    torch.save({"state_dict": sd}, path)
    m = vbx.VocosDecoder.from_checkpoint(path, hop_length=64, bandwidth_id=1)
    assert (m.input_channels, m.dim, m.num_layers, m.n_fft, m.hop_length) == (32, 64, 2, 256, 64) and not m.training
    got = m.state_dict()
    folded = 0
    for name in ["backbone.norm"] + [f"backbone.convnext.{i}.norm" for i in range(2)]:
        assert torch.equal(got[name + ".weight"], sd[name + ".scale.weight"][1]) and torch.equal(got[name + ".bias"], sd[name + ".shift.weight"][1])
        folded += 1
    assert folded == 3 and torch.equal(got["backbone.final_layer_norm.weight"], sd["backbone.final_layer_norm.weight"])
    assert not torch.equal(got["backbone.norm.weight"], sd["backbone.norm.scale.weight"][0])
    with pytest.raises(NotImplementedError, match="adanorm_num_embeddings"):
        vbx.VocosDecoder.from_checkpoint(path, hop_length=64)
    with pytest.raises(ValueError, match="bandwidth_id 9"):
        vbx.VocosDecoder.from_checkpoint(path, hop_length=64, bandwidth_id=9)
    with pytest.raises(NotImplementedError):
        vbx.VocosDecoder(input_channels=32, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64, adanorm_num_embeddings=4)


def test_from_vocos_checkpoint_round_trip(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = adanorm_state(1)
    path = str(tmp_path / "vocos_encodec.pt")
    torch.save(sd, path)
    codec = vbx.EncodecVocoCodec.from_vocos_checkpoint(path, bandwidth_id=1, codebook_size=16, hop_length=64)
    assert codec.rvq.num_quantizers == 4 and (codec.latent_dim, codec.downsample_factor, codec.sampling_rate) == (32, 64, 24000)
    assert torch.equal(codec.rvq.codebooks, sd["feature_extractor.codebook_weights"][:64].reshape(4, 16, 32))
    assert torch.equal(codec.vocoder.backbone.norm.bias.detach(), sd["backbone.norm.shift.weight"][1]) and not codec.training
    capped = vbx.EncodecVocoCodec.from_vocos_checkpoint(path, bandwidth_id=3, codebook_size=16, hop_length=64)
    assert capped.rvq.num_quantizers == 5  # id 3 asks for 16 codebooks, the table holds 5
    with pytest.raises(ValueError):
        vbx.EncodecVocoCodec.from_vocos_checkpoint(path, bandwidth_id=4, codebook_size=16)
    plain = str(tmp_path / "plain.pt")
    torch.save(vr.random_state(32, 64, 192, 2, 256, 0), plain)
    with pytest.raises(KeyError):
        vbx.EncodecVocoCodec.from_vocos_checkpoint(plain)
    # what the file holds comes back out of the module
    back = codec.state_dict()
    assert torch.equal(back["rvq.codebooks"].reshape(64, 32), sd["feature_extractor.codebook_weights"][:64])
    assert torch.equal(back["vocoder.head.out.weight"], sd["head.out.weight"])
