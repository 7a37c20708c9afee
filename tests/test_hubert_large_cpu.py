"""HubertLargeWithKmeans without a GPU: the restatement tests/hubert_large_ref.py against transformers.HubertModel itself in the large
form (feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias both ways) -- this PINS the yardstick of
tests/test_hubert_large_gpu.py --, the loaders, the cross-refusals of the two classes, the limits, the measured feature tolerances and
the code-agreement cap.  fairseq is absent: its large layout is translated as remembered and stays unpinned.

`python tests/test_hubert_large_cpu.py --write` writes the CPU half of profiles/hubert_large_parity.txt."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:  # run as a script (pytest's conftest.py has done this already)
        sys.path.insert(0, _p)

import hubert_large_ref as LR  # noqa: E402
import hubert_ref as R  # noqa: E402
from test_hubert_cpu import _to_fairseq, _without_placeholder_modules  # noqa: E402
from voicebox_pytorch_amd import HubertLargeWithKmeans, HubertWithKmeans  # noqa: E402
from voicebox_pytorch_amd.hubert import convert_state_dict  # noqa: E402


# ------------------------------------------------------------------------------------ 1. the restatement against the library
def _library_model(cfg, conv_bias):
    transformers = pytest.importorskip("transformers")
    hc = transformers.HubertConfig(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, feat_extract_norm="layer",
                                   do_stable_layer_norm=True, conv_bias=conv_bias, hidden_dropout=0.0, attention_dropout=0.0,
                                   activation_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
                                   mask_feature_prob=0.0, attn_implementation="eager")
    return transformers.HubertModel(hc).double().eval()


@pytest.mark.parametrize("conv_bias", [True, False])
@pytest.mark.parametrize("name", ["LSMALL", "LARGE6"])
def test_restatement_equals_transformers(name, conv_bias):
    """hidden_states[L] for every L within 1e-10 of transformers.HubertModel in fp64 (eager attention, no dropout, no masking): the
    un-normalised stream for L < n, encoder.layer_norm of it at L == n.  Random parameters with non-zero biases, loaded INTO the
    library's model under its own names"""
    cfg = LR.CFGS[name]
    sd = LR.random_state_dict(cfg, 3, torch.float64, conv_bias=conv_bias)
    wave = R.make_wave(2, 4000, 5)
    with _without_placeholder_modules(), torch.no_grad():
        model = _library_model(cfg, conv_bias)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k == "masked_spec_embed" for k in missing), (missing, unexpected)
        lib = model(wave.double(), output_hidden_states=True).hidden_states
    with torch.no_grad():
        mine = LR.hidden_states(sd, cfg, wave)
    assert len(lib) == len(mine) == cfg["num_hidden_layers"] + 1
    worst = [float((a - b).abs().max()) for a, b in zip(lib, mine)]
    print(name, "conv_bias", conv_bias, "max |delta| per hidden state:", " ".join(f"{w:.1e}" for w in worst))
    assert max(worst) < 1e-10
    assert mine[0].shape[1] == R.frames_of(4000, cfg) == 12
    # hidden_states[L] asked for alone is the same tensor: the final norm goes with L == n only
    with torch.no_grad():
        part = LR.hidden_states(sd, cfg, wave, upto=2)
    assert len(part) == 3 and float((part[2] - lib[2]).abs().max()) < 1e-10


# ------------------------------------------------------------------------------------ 2. loaders and limits
def _to_fairseq_large(sd):
    """fairseq's large layout AS REMEMBERED (the library is absent): Sequential(conv, dropout, Sequential(TransposeLast, LayerNorm,
    TransposeLast), gelu) -> the bias at conv_layers.{i}.0.bias, the norm at conv_layers.{i}.2.1.*"""
    special = {k: v for k, v in sd.items() if k.startswith("feature_extractor.") and not k.endswith(".conv.weight")}
    out = _to_fairseq({k: v for k, v in sd.items() if k not in special})
    for k, v in special.items():
        i, rest = k.split(".")[2], k.split(".", 3)[3]
        out[f"feature_extractor.conv_layers.{i}." + {"conv.bias": "0.bias", "layer_norm.weight": "2.1.weight", "layer_norm.bias": "2.1.bias"}[rest]] = v
    return out


@pytest.mark.parametrize("conv_bias", [True, False])
def test_loaders_agree(tmp_path, conv_bias):
    sd = LR.small_state_dict(conv_bias=conv_bias)
    hf = dict(sd, masked_spec_embed=torch.zeros(128))
    fs = _to_fairseq_large(sd)
    assert any(".2.1.weight" in k for k in fs) and (not conv_bias or "feature_extractor.conv_layers.3.0.bias" in fs)
    assert set(convert_state_dict(hf)) == set(sd) == set(convert_state_dict(fs)) == set(convert_state_dict({"model": fs}))
    for variant in (hf, fs, {"model": fs}, {"hubert." + k: v for k, v in sd.items()}):
        m = HubertLargeWithKmeans(**LR.LSMALL, output_layer=2, codebook_size=64, conv_bias=conv_bias)
        m.load_state_dict(variant)
        got = {k: v for k, v in m.state_dict().items() if k != "cluster_centers"}
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    centers = torch.randn(64, 128, generator=torch.Generator().manual_seed(1))
    torch.save(centers, tmp_path / "km.pt")
    for i, variant in enumerate((sd, {"model": fs})):
        torch.save(variant, tmp_path / f"h{i}.pt")
        m = HubertLargeWithKmeans.from_checkpoint(tmp_path / f"h{i}.pt", tmp_path / "km.pt", output_layer=3, normalize_wave=True)
        assert {k: getattr(m, k) for k in LR.LSMALL} == LR.LSMALL and m.output_layer == 3 and m.codebook_size == 64 and not m.training
        assert (m.conv_bias, m.feat_extract_norm, m.do_stable_layer_norm, m.normalize_wave, m.normalize_eps) == (conv_bias, "layer", True, True, 1e-7)
        assert torch.equal(m.cluster_centers, centers) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
        assert (m.target_sample_hz, m.downsample_factor, m.groups) == (16000, 320, 1) and not any(p.requires_grad for p in m.parameters())
    assert not HubertLargeWithKmeans.from_state_dict(sd, centers, output_layer=1).normalize_wave  # the default: audiolm_pytorch's module does not normalise
    # the library's own state_dict() loads as is
    with _without_placeholder_modules():
        lib = _library_model(LR.LSMALL, conv_bias)
        m = HubertLargeWithKmeans.from_state_dict(lib.state_dict(), centers, output_layer=4)
    assert m.conv_bias == conv_bias and m.num_hidden_layers == 4
    assert all(torch.equal(v, lib.state_dict()[k].float()) for k, v in m.state_dict().items() if k != "cluster_centers")


def test_base_dicts_convert_as_before():
    """the translation of a base dict did not move: the same keys and tensors from all four layouts"""
    sd = R.small_state_dict()
    for variant in (sd, _to_fairseq(sd), {"model": _to_fairseq(sd)}):
        got = convert_state_dict(variant)
        assert set(got) == set(sd) and all(got[k] is sd[k] for k in sd)


def test_the_two_classes_refuse_each_others_files():
    centers = torch.zeros(64, 128)
    base, large = R.small_state_dict(), LR.small_state_dict()
    with pytest.raises(ValueError, match="HubertWithKmeans"):
        HubertLargeWithKmeans.from_state_dict(base, centers)
    with pytest.raises(ValueError, match="HubertWithKmeans"):
        HubertLargeWithKmeans.from_state_dict(_to_fairseq(base), centers)
    mixed = dict(base, **{k: v for k, v in large.items() if k.endswith(".conv.bias") and k.startswith("feature_extractor.")})
    with pytest.raises(ValueError, match="neither this class nor HubertWithKmeans"):  # biases without per-layer norms: nobody's file
        HubertLargeWithKmeans.from_state_dict(mixed, centers)
    with pytest.raises(NotImplementedError, match="conv_bias"):
        HubertWithKmeans.from_state_dict(mixed, centers)
    for sd in (large, LR.small_state_dict(conv_bias=False), _to_fairseq_large(large)):
        with pytest.raises(NotImplementedError, match="HubertLargeWithKmeans"):
            HubertWithKmeans.from_state_dict(sd, centers)
    # the old constructor's refusals now name the new class (and still say what tests/test_hubert_cpu.py matches)
    for kw, word in ((dict(feat_extract_norm="layer"), "feat_extract_norm"), (dict(do_stable_layer_norm=True), "do_stable_layer_norm"),
                     (dict(conv_bias=True), "conv_bias")):
        with pytest.raises(NotImplementedError, match=word) as ei:
            HubertWithKmeans(**kw)
        assert "HubertLargeWithKmeans" in str(ei.value)


def test_defaults_are_hubert_large_ll60k():
    import inspect

    d = {k: v.default for k, v in inspect.signature(HubertLargeWithKmeans.__init__).parameters.items() if k != "self"}
    assert (d["hidden_size"], d["num_hidden_layers"], d["num_attention_heads"], d["intermediate_size"]) == (1024, 24, 16, 4096)
    assert (d["conv_dim"], d["conv_kernel"], d["conv_stride"]) == ((512,) * 7, (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))
    assert (d["num_conv_pos_embeddings"], d["num_conv_pos_embedding_groups"]) == (128, 16)
    assert (d["feat_extract_norm"], d["do_stable_layer_norm"], d["conv_bias"], d["normalize_wave"], d["normalize_eps"]) == ("layer", True, True, False, 1e-7)
    b = {k: v.default for k, v in inspect.signature(HubertWithKmeans.__init__).parameters.items() if k != "self"}
    same = [k for k in b if k not in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "feat_extract_norm",
                                      "do_stable_layer_norm", "conv_bias")]
    assert all(d[k] == b[k] for k in same)
    m = HubertLargeWithKmeans(**LR.LSMALL, output_layer=4, codebook_size=64)
    names = set(m.state_dict())
    assert all(f"feature_extractor.conv_layers.{i}.{n}" in names for i in range(7) for n in ("conv.bias", "layer_norm.weight", "layer_norm.bias"))
    assert "feature_extractor.conv_layers.1.conv.bias" not in HubertLargeWithKmeans(**LR.LSMALL, output_layer=4, conv_bias=False).state_dict()


FORMS = [dict(feat_extract_norm="group"), dict(do_stable_layer_norm=False), dict(feat_extract_norm="group", do_stable_layer_norm=False),
         dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)]
LIMITS = [(dict(hidden_size=1280, num_attention_heads=16), "must be 64"), (dict(hidden_size=96, num_attention_heads=1), "must be 64"),
          (dict(hidden_size=2112, num_attention_heads=33), "at most 2048"), (dict(conv_dim=(512,) * 6 + (256,)), "conv_dim"),
          (dict(conv_dim=(24,) * 7), "conv_dim"), (dict(conv_dim=(1024,) * 7), "conv_dim"), (dict(conv_kernel=(20, 3, 3, 3, 3, 2, 2)), r"conv_kernel\[0\]"),
          (dict(conv_kernel=(10, 3, 3, 4, 3, 2, 2)), "2 or 3"), (dict(conv_stride=(5, 2, 2, 3, 2, 2, 2)), "conv_stride"),
          (dict(num_conv_pos_embedding_groups=256), "multiple of 8"), (dict(num_conv_pos_embeddings=127), "even"),
          (dict(codebook_size=1), "codebook_size"), (dict(codebook_size=4097), "codebook_size"), (dict(output_layer=0), "output_layer"),
          (dict(output_layer=25), "output_layer")]


@pytest.mark.parametrize("kw", FORMS, ids=[str(i) for i in range(len(FORMS))])
def test_other_forms_raise_and_name_the_base_class(kw):
    with pytest.raises(NotImplementedError, match="HubertWithKmeans serves"):
        HubertLargeWithKmeans(**kw)


@pytest.mark.parametrize("kw,match", LIMITS, ids=[f"{i}-{m[:12]}" for i, (_, m) in enumerate(LIMITS)])
def test_limits_raise_at_construction(kw, match):
    """every other limit is the base class's, raised before anything touches a device; x-large (head size 80) keeps raising"""
    with pytest.raises(NotImplementedError, match=match) as ei:
        HubertLargeWithKmeans(**kw)
    assert str(ei.value).startswith("HubertLargeWithKmeans:")


def test_cpu_tensors_and_masks_are_refused():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd._lib import VbxError

    for nw in (False, True):
        m = HubertLargeWithKmeans(**LR.LSMALL, output_layer=2, codebook_size=64, normalize_wave=nw)
        with pytest.raises(VbxError):
            m(torch.zeros(1, 4000))
        with pytest.raises(VbxError):
            m.features(torch.zeros(1, 1, 4000), lens=[4000])
        with pytest.raises(NotImplementedError, match="mask"):
            m(torch.zeros(1, 4000), attention_mask=torch.ones(1, 4000))
    with pytest.raises(VbxError):
        vbx.normalize_wave(torch.zeros(2, 100))
    with pytest.raises(ValueError, match=r"lens\[1\] = 101"):
        vbx.normalize_wave(torch.zeros(2, 100), lens=[100, 101])
    with pytest.raises(ValueError, match="eps"):
        vbx.normalize_wave(torch.zeros(2, 100), eps=0.0)


def test_wrapper_keyword_on_the_host():
    import voicebox_pytorch_amd as vbx

    kw = dict(dim=64, num_cond_tokens=64, depth=2, dim_head=64, heads=2, time_hidden_dim=64, ff_mult=2)
    tok = HubertLargeWithKmeans(**LR.LSMALL, output_layer=2, codebook_size=64)
    w = vbx.ConditionalFlowMatcherWrapper(voicebox=vbx.VoiceBox(condition_on_text=True, **kw), wav2vec=tok)
    assert w.wav2vec is tok and "wav2vec.cluster_centers" in w.state_dict() and not any(p.requires_grad for p in tok.parameters())
    from voicebox_pytorch_amd.wave_lens import wav2vec_lacks

    assert wav2vec_lacks(tok) is None  # lens= and frame_lens: it serves wave_lens= like the base class


# ------------------------------------------------------------------------------------ 3. the tolerances, measured
WAVES = (400, 719, 720, 5000)  # the GPU test's lengths


def _emulated_distance(layer):
    sd = LR.small_state_dict()
    worst = 0.0
    with torch.no_grad():
        for T in WAVES:
            wave = R.make_wave(2, T, 20 + T % 97)
            worst = max(worst, R.movement(LR.features(sd, LR.LSMALL, wave, layer, emulate=True), LR.features(sd, LR.LSMALL, wave, layer)))
    return worst


@pytest.mark.parametrize("layer", [2, 4])
def test_tolerance_is_a_tenth_of_the_smallest_fault(layer):
    """measured once for output_layer < n (the un-normalised branch) and once for output_layer == n (the final norm); the emulated
    restatement alone must be inside it, or the inputs are wrong"""
    tol, table = LR.tolerance_small(layer)
    want = LR.FAULTS_END if layer == 4 else LR.FAULTS_MID
    assert set(table) == set(want) and len(want) == 8 and all(v > 0 for v in table.values())
    assert tol == min(table.values()) / 10
    emu = _emulated_distance(layer)
    print(f"layer {layer}: tolerance {tol:.4e}, emulated restatement's own distance from fp64 {emu:.4e}")
    assert emu < tol


def test_faults_that_do_not_apply_move_nothing():
    """ln_every_state is the right network at L == n and no_final_ln at L < n: why each is left out of the other minimum"""
    sd, wave = LR.small_state_dict(), R.make_wave(1, 2000, 2)
    with torch.no_grad():
        assert torch.equal(LR.features(sd, LR.LSMALL, wave, 4, fault="ln_every_state"), LR.features(sd, LR.LSMALL, wave, 4))
        assert torch.equal(LR.features(sd, LR.LSMALL, wave, 2, fault="no_final_ln"), LR.features(sd, LR.LSMALL, wave, 2))


# ------------------------------------------------------------------------------------ 4. code agreement: a cap
CODE_SEED = 77


def _flips():
    sd = LR.small_state_dict()
    wave = R.make_wave(2, 400 + 320 * 98, CODE_SEED)  # the GPU test's input: 2 x 99 frames
    c = LR.codebook("LSMALL", 0, 4, 64)
    with torch.no_grad():
        ref, emu = LR.features(sd, LR.LSMALL, wave, 4), LR.features(sd, LR.LSMALL, wave, 4, emulate=True)
    a, b = R.kmeans_assign(ref, c)[0], R.kmeans_assign(emu, c)[0]
    assert a.numel() == 198
    return float((a != b).float().mean()), len(a.unique())


def test_code_agreement_of_the_emulated_restatement():
    """the GPU test allows 5 % of 198 frames to differ from the fp64 argmin: fp16 operands alone must stay within it on that wave and
    seed, and the codes must not have collapsed onto a few centres"""
    flips, used = _flips()
    print(f"LSMALL: {flips * 100:.2f} % of 198 frames flip, {used} of 64 codes in use")
    assert flips <= 0.05 and used >= 16


def test_normalize_restatement_is_the_preprocessors():
    """hubert_large_ref.normalize against transformers' Wav2Vec2FeatureExtractor (do_normalize=True), rows of unequal length"""
    transformers = pytest.importorskip("transformers")
    np = pytest.importorskip("numpy")
    wave = (R.make_wave(2, 3000, 6) + 0.3).double()
    lens = [3000, 1777]
    with _without_placeholder_modules():
        fe = transformers.Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=True)
        out = fe([wave[b, :l].numpy().astype(np.float64) for b, l in enumerate(lens)], sampling_rate=16000, padding=True, return_tensors="np")
    got = LR.normalize(wave, lens)
    assert float((torch.from_numpy(np.asarray(out["input_values"], dtype=np.float64)) - got).abs().max()) < 1e-5  # the library works in fp32
    assert (got[1, 1777:] == 0).all()


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "hubert_large_parity.txt")
    lines = ["HubertLargeWithKmeans: feature tolerances as measured (tests/hubert_large_ref.py, tests/test_hubert_large_cpu.py), max |delta| / RMS",
             "at LSMALL (hubert_ref.SMALL's widths in the large form, conv_bias on), B 2, T 5000.  Each planted fault's movement of the fp64 restatement:"]
    for layer, what in ((2, "hidden_states[2] of 4: the un-normalised stream"), (4, "hidden_states[4] of 4: encoder.layer_norm applied")):
        tol, table = LR.tolerance_small(layer)
        lines += [f"{what}"] + [f"  {f:22s} {v:.4e}" for f, v in table.items()]
        lines += [f"  tolerance = smallest movement / 10 = {tol:.4e}",
                  f"  emulated restatement (fp16 roundings as include/vbx.h states them) from fp64, worst of T {' / '.join(map(str, WAVES))}: {_emulated_distance(layer):.4e}"]
    flips, used = _flips()
    lines.append(f"code flips of the emulated restatement, LSMALL layer 4 K 64, wave seed {CODE_SEED}: {flips * 100:.2f} % of 198 frames ({used} codes in use)")
    text = "\n".join(lines) + "\n"
    if "--write" in sys.argv:
        with open(out, "w") as fh:
            fh.write(text)
    print(text)
