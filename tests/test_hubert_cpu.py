"""HubertWithKmeans without a GPU: the restatement tests/hubert_ref.py against transformers.HubertModel itself (this PINS the yardstick
of tests/test_hubert_gpu.py against a library), the loaders, the limits, the measured feature tolerance and the code-agreement cap.

`python tests/test_hubert_cpu.py` writes the CPU half of profiles/hubert_parity.txt (the fault table and the emulated distance)."""
import contextlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run as a script (pytest's conftest.py has done this already)
    sys.path.insert(0, ROOT)

import hubert_ref as R  # noqa: E402
from voicebox_pytorch_amd import HubertWithKmeans  # noqa: E402
from voicebox_pytorch_amd.hubert import convert_state_dict, load_kmeans  # noqa: E402


# ------------------------------------------------------------------------------------ 1. the restatement against the library
@contextlib.contextmanager
def _without_placeholder_modules():
    """The oracle's loader leaves placeholder modules (torchaudio, vocos, ...) without a __spec__ in sys.modules for the rest of a
    session; transformers probes its optional packages with importlib.util.find_spec, which raises ValueError on such an entry."""
    names = ("beartype", "torchdiffeq", "torchode", "naturalspeech2_pytorch", "audiolm_pytorch", "spear_tts_pytorch", "gateloop_transformer",
             "torchaudio", "vocos")
    hidden = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in names and getattr(sys.modules[k], "__spec__", 0) is None}
    try:
        yield
    finally:
        sys.modules.update(hidden)


def _library_model(cfg):
    transformers = pytest.importorskip("transformers")
    hc = transformers.HubertConfig(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, feat_extract_norm="group",
                                   do_stable_layer_norm=False, conv_bias=False, hidden_dropout=0.0, attention_dropout=0.0,
                                   activation_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
                                   mask_feature_prob=0.0, attn_implementation="eager")
    return transformers.HubertModel(hc).double().eval()


@pytest.mark.parametrize("name", ["SMALL", "BASE"])
def test_restatement_equals_transformers(name):
    """hidden_states[L] for every L within 1e-10 of transformers.HubertModel in fp64 (eager attention, no dropout, no masking); the
    parameters are random from a seed with non-zero biases, loaded INTO the library's model under its own names"""
    cfg = dict(SMALL=R.SMALL, BASE=R.BASE)[name]
    sd = R.random_state_dict(cfg, 3, torch.float64)
    wave = R.make_wave(2, 4000, 5)
    with _without_placeholder_modules(), torch.no_grad():
        model = _library_model(cfg)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k == "masked_spec_embed" for k in missing), (missing, unexpected)
        lib = model(wave.double(), output_hidden_states=True).hidden_states
    with torch.no_grad():
        mine = R.hidden_states(sd, cfg, wave)
    assert len(lib) == len(mine) == cfg["num_hidden_layers"] + 1
    worst = [float((a - b).abs().max()) for a, b in zip(lib, mine)]
    print(name, "max |delta| per hidden state:", " ".join(f"{w:.1e}" for w in worst))
    assert max(worst) < 1e-10
    assert mine[0].shape[1] == R.frames_of(4000, cfg) == 12


# ------------------------------------------------------------------------------------ 2. loaders and limits
def _to_fairseq(sd):
    out = {}
    for k, v in sd.items():
        k = k.replace("feature_projection.layer_norm.", "layer_norm.").replace("feature_projection.projection.", "post_extract_proj.")
        k = k.replace(".conv.weight", ".0.weight") if k.startswith("feature_extractor.") else k
        k = k.replace("conv_layers.0.layer_norm.", "conv_layers.0.2.")
        k = k.replace("encoder.pos_conv_embed.conv.parametrizations.weight.original0", "encoder.pos_conv.0.weight_g")
        k = k.replace("encoder.pos_conv_embed.conv.parametrizations.weight.original1", "encoder.pos_conv.0.weight_v")
        k = k.replace("encoder.pos_conv_embed.conv.bias", "encoder.pos_conv.0.bias")
        if k.startswith("encoder.layers."):
            k = k.replace(".attention.", ".self_attn.").replace(".feed_forward.intermediate_dense.", ".fc1.").replace(".feed_forward.output_dense.", ".fc2.")
            parts = k.split(".")
            if parts[3] == "layer_norm":
                k = ".".join(parts[:3] + ["self_attn_layer_norm"] + parts[4:])
        out[k] = v
    out.update(mask_emb=torch.zeros(4), label_embs_concat=torch.zeros(3, 4))
    out["final_proj.weight"], out["final_proj.bias"] = torch.zeros(4, 4), torch.zeros(4)
    return out


def test_loaders_agree(tmp_path):
    sd = R.small_state_dict()
    hf = dict(sd, masked_spec_embed=torch.zeros(128))
    old = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): v for k, v in sd.items()}
    assert set(convert_state_dict(hf)) == set(sd) == set(convert_state_dict(_to_fairseq(sd))) == set(convert_state_dict(old))
    want = None
    for variant in (hf, _to_fairseq(sd), old, {"model": _to_fairseq(sd)}, {"hubert." + k: v for k, v in sd.items()}):
        m = HubertWithKmeans(**R.SMALL, output_layer=2, codebook_size=64)
        m.load_state_dict(variant)
        got = {k: v.clone() for k, v in m.state_dict().items() if k != "cluster_centers"}
        assert set(got) == set(sd)
        want = got if want is None else want
        assert all(torch.equal(got[k], want[k]) and torch.equal(got[k], sd[k]) for k in sd)
    # from_checkpoint: every width off the shapes, from both layouts; k-means as a tensor, a .npy and a joblib'd sklearn estimator
    centers = torch.randn(64, 128, generator=torch.Generator().manual_seed(1))
    torch.save(centers, tmp_path / "km.pt")
    for i, variant in enumerate((sd, {"model": _to_fairseq(sd)})):
        torch.save(variant, tmp_path / f"h{i}.pt")
        m = HubertWithKmeans.from_checkpoint(tmp_path / f"h{i}.pt", tmp_path / "km.pt", output_layer=3)
        cfg = {k: getattr(m, k) for k in R.SMALL}
        assert cfg == R.SMALL and m.output_layer == 3 and m.codebook_size == 64 and not m.training
        assert torch.equal(m.cluster_centers, centers) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
        assert (m.target_sample_hz, m.downsample_factor, m.groups, m.seq_len_multiple_of) == (16000, 320, 1, None)
        assert not any(p.requires_grad for p in m.parameters())
    assert [m.frames(t) for t in (399, 400, 719, 720, 16000)] == [0, 1, 1, 2, 49]
    np = pytest.importorskip("numpy")
    np.save(tmp_path / "km.npy", centers.numpy())
    assert torch.equal(load_kmeans(tmp_path / "km.npy"), centers)
    cluster, joblib = pytest.importorskip("sklearn.cluster"), pytest.importorskip("joblib")
    km = cluster.MiniBatchKMeans(n_clusters=8, n_init=1, random_state=0).fit(torch.randn(200, 128, generator=torch.Generator().manual_seed(2)).numpy())
    joblib.dump(km, tmp_path / "km.bin")
    got = load_kmeans(tmp_path / "km.bin")
    assert got.dtype == torch.float32 and torch.equal(got, torch.as_tensor(km.cluster_centers_).float())
    m = HubertWithKmeans.from_checkpoint(tmp_path / "h0.pt", tmp_path / "km.bin", output_layer=1)
    assert m.codebook_size == 8 and torch.equal(m.cluster_centers, got)


LIMITS = [(dict(feat_extract_norm="layer"), "feat_extract_norm"), (dict(do_stable_layer_norm=True), "do_stable_layer_norm"),
          (dict(conv_bias=True), "conv_bias"), (dict(hidden_size=1280, num_attention_heads=16), "must be 64"),
          (dict(hidden_size=96, num_attention_heads=1), "must be 64"), (dict(hidden_size=2112, num_attention_heads=33), "at most 2048"),
          (dict(conv_dim=(512,) * 6 + (256,)), "conv_dim"), (dict(conv_dim=(24,) * 7), "conv_dim"), (dict(conv_dim=(1024,) * 7), "conv_dim"),
          (dict(conv_kernel=(20, 3, 3, 3, 3, 2, 2)), r"conv_kernel\[0\]"), (dict(conv_kernel=(10, 3, 3, 4, 3, 2, 2)), "2 or 3"),
          (dict(conv_kernel=(10, 3, 3, 1, 3, 2, 2)), "2 or 3"), (dict(conv_stride=(5, 2, 2, 3, 2, 2, 2)), "conv_stride"),
          (dict(num_conv_pos_embedding_groups=64), "multiple of 8"), (dict(num_conv_pos_embeddings=127), "even"),
          (dict(codebook_size=1), "codebook_size"), (dict(codebook_size=4097), "codebook_size"),
          (dict(output_layer=0), "output_layer"), (dict(output_layer=13), "output_layer")]


@pytest.mark.parametrize("kw,match", LIMITS, ids=[f"{i}-{m[:12]}" for i, (_, m) in enumerate(LIMITS)])
def test_limits_raise_at_construction(kw, match):
    """every limit names itself in a NotImplementedError before anything touches a device"""
    with pytest.raises(NotImplementedError, match=match):
        HubertWithKmeans(**kw)


def test_cpu_tensors_and_masks_are_refused():
    from voicebox_pytorch_amd._lib import VbxError

    m = HubertWithKmeans(**R.SMALL, output_layer=2, codebook_size=64)
    with pytest.raises(VbxError):
        m(torch.zeros(1, 4000))
    with pytest.raises(VbxError):
        m.features(torch.zeros(1, 1, 4000))
    with pytest.raises(NotImplementedError, match="mask"):
        m(torch.zeros(1, 4000), attention_mask=torch.ones(1, 4000))


def test_wrapper_keyword_on_the_host():
    """wav2vec= is a new keyword: a frozen submodule of a text-conditioned wrapper; text_to_semantic= keeps raising"""
    import voicebox_pytorch_amd as vbx

    kw = dict(dim=64, num_cond_tokens=64, depth=2, dim_head=64, heads=2, time_hidden_dim=64, ff_mult=2)
    tok = HubertWithKmeans(**R.SMALL, output_layer=2, codebook_size=64)
    w = vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(condition_on_text=True, **kw), wav2vec=tok)
    assert w.wav2vec is tok and "wav2vec.cluster_centers" in w.state_dict() and not any(p.requires_grad for p in tok.parameters())
    assert vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(condition_on_text=True, **kw)).wav2vec is None
    with pytest.raises(NotImplementedError, match="TextToSemantic"):
        vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(condition_on_text=True, **kw), text_to_semantic=object())
    with pytest.raises(AssertionError):
        vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(condition_on_text=False, **kw), wav2vec=tok)
    with pytest.raises(TypeError, match="target_sample_hz"):
        vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(condition_on_text=True, **kw), wav2vec=object())


# ------------------------------------------------------------------------------------ 3. the tolerance, measured
def _emulated_distance():
    sd = R.small_state_dict()
    worst = 0.0
    with torch.no_grad():
        for T in (400, 720, 5000, 41360):
            wave = R.make_wave(2, T, 20 + T % 97)
            worst = max(worst, R.movement(R.features(sd, R.SMALL, wave, 4, emulate=True), R.features(sd, R.SMALL, wave, 4)))
    return worst


def test_tolerance_is_a_tenth_of_the_smallest_fault():
    tol, table = R.tolerance_small()
    assert len(R.FAULTS) >= 8 and all(table[f] > 0 for f in R.FAULTS + R.SOFT_FAULTS)
    assert tol == min(table[f] for f in R.FAULTS) / 10
    emu = _emulated_distance()
    print(f"tolerance {tol:.4e}, emulated restatement's own distance from fp64 {emu:.4e}")
    assert emu < tol  # fp16 operands alone must leave room


# ------------------------------------------------------------------------------------ 4. code agreement: a cap
def _flips(name, cfg, layer, K):
    sd = R.small_state_dict() if name == "SMALL" else R.base_state_dict()
    wave = R.make_wave(2, 400 + 320 * 98, 77)  # the GPU test's input: 2 x 99 frames
    c = R.codebook(name, 0, layer, K)
    with torch.no_grad():
        ref, emu = R.features(sd, cfg, wave, layer), R.features(sd, cfg, wave, layer, emulate=True)
    a, b = R.kmeans_assign(ref, c)[0], R.kmeans_assign(emu, c)[0]
    assert a.numel() == 198
    return float((a != b).float().mean()), len(a.unique())


def test_code_agreement_of_the_emulated_restatement_small():
    """the GPU test allows 5 % of frames to differ from the fp64 argmin; fp16 operands alone (the emulated restatement) must stay
    within 1 %, and the codes must not have collapsed onto a few centres"""
    flips, used = _flips("SMALL", R.SMALL, 4, 64)
    print(f"SMALL: {flips * 100:.2f} % of 198 frames flip, {used} of 64 codes in use")
    assert flips <= 0.01 and used >= 16


def test_code_agreement_of_the_emulated_restatement_base():
    flips, used = _flips("BASE", R.BASE, 9, 500)
    print(f"BASE layer 9: {flips * 100:.2f} % of 198 frames flip, {used} of 500 codes in use")
    assert flips <= 0.01 and used >= 32


if __name__ == "__main__":
    tol, table = R.tolerance_small()
    out = os.path.join(ROOT, "profiles", "hubert_parity.txt")
    lines = ["HubertWithKmeans: feature tolerance as measured (tests/hubert_ref.py, tests/test_hubert_cpu.py), max |delta| / RMS at SMALL,",
             "hidden_states[4], B 2, T 5000.  Each planted fault's movement of the fp64 restatement:"]
    lines += [f"  {f:22s} {table[f]:.4e}" for f in R.FAULTS]
    lines += ["approximation-level perturbations (below fp16 resolution, not part of the minimum):"]
    lines += [f"  {f:22s} {table[f]:.4e}" for f in R.SOFT_FAULTS]
    lines += [f"tolerance = smallest structural movement / 10 = {tol:.4e}",
              f"emulated restatement (fp16 roundings as include/vbx.h states them) from fp64, worst of T 400 / 720 / 5000 / 41360: {_emulated_distance():.4e}"]
    for name, cfg, layer, K in (("SMALL", R.SMALL, 4, 64), ("BASE", R.BASE, 9, 500)):
        flips, used = _flips(name, cfg, layer, K)
        lines.append(f"code flips of the emulated restatement, {name} layer {layer} K {K}: {flips * 100:.2f} % of 198 frames ({used} codes in use)")
    text = "\n".join(lines) + "\n"
    if "--write" in sys.argv:
        with open(out, "w") as fh:
            fh.write(text)
    print(text)
