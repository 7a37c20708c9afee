"""HuBERT LARGE (feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias either way) restated in fp64 from F.conv1d /
F.layer_norm / F.gelu / softmax with transformers.HubertModel's parameter names -- the yardstick of
voicebox_pytorch_amd.HubertLargeWithKmeans.  tests/test_hubert_large_cpu.py holds it against the library itself (1e-10 at every hidden
state, bias on and off), so it is PINNED like tests/hubert_ref.py, whose helpers it shares.

hidden_states[L] as the library names them: the UN-normalised residual stream after layer L for L < num_hidden_layers, and
encoder.layer_norm of it for L == num_hidden_layers only.

emulate=True rounds operands and stored activations to fp16 exactly where include/vbx.h ("THE LARGE FORM") says the kernels do, and
nowhere else; all sums stay fp64.  Not mirrored: fp32 summation order, the fp16 probabilities inside vbx_attn_fwd, the
Abramowitz-Stegun erf of VBX_EPI_GELU.

fault=NAME plants one structural error; a tenth of the smallest movement among those that apply to the layer asked for is the
tolerance of the feature tests (tolerance_small)."""
import functools
import math

import torch
import torch.nn.functional as F

import hubert_ref as R
from hubert_ref import G0, G1, LOG2E, fold_weight_norm, frames_of, kmeans_assign, kmeans_bound, make_wave, movement, r16  # noqa: F401

LSMALL = dict(R.SMALL)  # hubert_ref.SMALL's widths in the large form
LARGE6 = dict(hidden_size=1024, num_hidden_layers=6, num_attention_heads=16, intermediate_size=4096, conv_dim=(512,) * 7,
              conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=128,
              num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5)
CFGS = dict(LSMALL=LSMALL, LARGE6=LARGE6)

# every fault is a different network.  ln_every_state moves only hidden_states[L < n], no_final_ln only hidden_states[n].
FAULTS = ("norm_over_time", "conv_bias_dropped", "post_ln", "encoder_ln_after_pos", "ln_every_state", "no_final_ln", "ffn_norm_skipped",
          "prev_hidden", "gn_first_layer")
FAULTS_MID = tuple(f for f in FAULTS if f != "no_final_ln")      # what can go wrong where output_layer < num_hidden_layers
FAULTS_END = tuple(f for f in FAULTS if f != "ln_every_state")   # ... and where output_layer == num_hidden_layers


def random_state_dict(cfg, seed, dtype=torch.float32, conv_bias=True):
    """hubert_ref.random_state_dict's parameters plus what the large form adds: a LayerNorm for every convolution after the first
    (gains around one, biases of std 0.2) and, with conv_bias, a bias of std 0.3 on every convolution"""
    sd = R.random_state_dict(cfg, seed, torch.float64)
    g = torch.Generator().manual_seed(seed + 1000)
    C = cfg["conv_dim"][0]
    for i in range(len(cfg["conv_kernel"])):
        p = f"feature_extractor.conv_layers.{i}."
        if i >= 1:
            sd[p + "layer_norm.weight"] = 0.75 + 0.5 * torch.rand(C, generator=g, dtype=torch.float64)
            sd[p + "layer_norm.bias"] = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
        if conv_bias:
            sd[p + "conv.bias"] = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    return {k: v.to(dtype) for k, v in sd.items()}


def hidden_states(sd, cfg, wave, upto=None, emulate=False, fault=None):
    """[hidden_states[0], ..., hidden_states[upto]] as transformers.HubertModel(output_hidden_states=True) names them for the large
    form, fp64 [B, N, D].  conv_bias is read off the keys."""
    assert fault is None or fault in FAULTS, fault
    e = emulate
    p = lambda n: sd[n].double()
    eps, C, D, H = cfg["layer_norm_eps"], cfg["conv_dim"][0], cfg["hidden_size"], cfg["num_attention_heads"]
    n_layers = cfg["num_hidden_layers"]
    L = n_layers if upto is None else upto
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), p(n + ".weight"), p(n + ".bias"), eps)
    x = wave.double()[:, None, :]
    for i in range(len(cfg["conv_kernel"])):
        pre = f"feature_extractor.conv_layers.{i}."
        w = p(pre + "conv.weight")
        bias = p(pre + "conv.bias") if pre + "conv.bias" in sd and fault != "conv_bias_dropped" else None
        x = F.conv1d(x, r16(w, e and i > 0), bias, stride=cfg["conv_stride"][i])  # the first convolution's weights stay fp32
        if fault == "norm_over_time" or (fault == "gn_first_layer" and i == 0):
            x = F.group_norm(x, C, p(pre + "layer_norm.weight"), p(pre + "layer_norm.bias"), eps)
        else:
            x = ln(x.transpose(1, 2), pre + "layer_norm").transpose(1, 2)
        x = r16(F.gelu(x), e)
    x = x.transpose(1, 2)
    x = r16(ln(x, "feature_projection.layer_norm"), e) @ r16(p("feature_projection.projection.weight"), e).t() + p("feature_projection.projection.bias")
    k = cfg["num_conv_pos_embeddings"]
    w = r16(fold_weight_norm(sd[G0], sd[G1], e), e)
    pos = F.conv1d(r16(x, e).transpose(1, 2), w, p("encoder.pos_conv_embed.conv.bias"), padding=k // 2, groups=cfg["num_conv_pos_embedding_groups"])[..., :-1]
    x = x + F.gelu(pos).transpose(1, 2)
    if fault == "encoder_ln_after_pos":
        x = ln(x, "encoder.layer_norm")
    hs = []
    scale = (D // H) ** -0.5
    B, N, _ = x.shape
    heads = lambda t: t.view(B, N, H, D // H).transpose(1, 2)
    for l in range(L):
        hs.append(ln(x, "encoder.layer_norm") if fault == "ln_every_state" else x)
        pre = f"encoder.layers.{l}."
        lin = lambda t, n: t @ r16(p(pre + n + ".weight"), e).t() + p(pre + n + ".bias")

        def attn(t):
            t16 = r16(t, e)
            q, kk, v = lin(t16, "attention.q_proj") * scale, lin(t16, "attention.k_proj"), lin(t16, "attention.v_proj")
            if e:  # q16 = fp16(q * scale * log2(e)), the attention kernels' contract
                logits = (heads(r16(q * LOG2E, e)) @ heads(r16(kk, e)).transpose(-1, -2)) / LOG2E
            else:
                logits = heads(q) @ heads(kk).transpose(-1, -2)
            o = torch.softmax(logits, -1) @ heads(r16(v, e))
            return lin(r16(o.transpose(1, 2).reshape(B, N, D), e), "attention.out_proj")

        ff = lambda t: lin(r16(F.gelu(lin(r16(t, e), "feed_forward.intermediate_dense")), e), "feed_forward.output_dense")
        if fault == "post_ln":
            x = ln(x + attn(x), pre + "layer_norm")
            x = ln(x + ff(x), pre + "final_layer_norm")
        else:
            x = x + attn(ln(x, pre + "layer_norm"))
            x = x + ff(x if fault == "ffn_norm_skipped" else ln(x, pre + "final_layer_norm"))
    last = L == n_layers
    if fault == "encoder_ln_after_pos":
        hs.append(x)
    elif fault == "ln_every_state":
        hs.append(ln(x, "encoder.layer_norm"))
    elif fault == "no_final_ln":
        hs.append(x)
    else:
        hs.append(ln(x, "encoder.layer_norm") if last else x)
    return hs


def features(sd, cfg, wave, layer, emulate=False, fault=None):
    """hidden_states[layer], fp64 [B, N, D]; the fault "prev_hidden" answers with hidden_states[layer - 1]"""
    hs = hidden_states(sd, cfg, wave, upto=layer, emulate=emulate, fault=fault)
    return hs[layer - 1] if fault == "prev_hidden" else hs[layer]


def normalize(wave, lens=None, eps=1e-7):
    """transformers' Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm in fp64: per row (x - mean) / sqrt(var + eps), biased variance,
    over the row's own samples; zeros past them"""
    x = wave.double()
    out = torch.zeros_like(x)
    for b in range(x.shape[0]):
        l = x.shape[1] if lens is None else int(lens[b])
        r = x[b, :l]
        out[b, :l] = (r - r.mean()) / torch.sqrt(r.var(unbiased=False) + eps)
    return out


@functools.lru_cache(maxsize=None)
def _cached_sd(name, seed, conv_bias):
    return random_state_dict(CFGS[name], seed, conv_bias=conv_bias)


def small_state_dict(seed=0, conv_bias=True):
    return _cached_sd("LSMALL", seed, conv_bias)


def large6_state_dict(seed=0):
    return _cached_sd("LARGE6", seed, True)


@functools.lru_cache(maxsize=None)
def codebook(name, seed, layer, K, frames_per_wave=99):
    """hubert_ref.codebook for the large form: K feature frames of OTHER waves through the same network, fp32 [K, D]"""
    cfg, sd = CFGS[name], _cached_sd(name, seed, True)
    T = 400 + 320 * (frames_per_wave - 1)
    rows, s = [], 1000
    with torch.no_grad():
        while sum(r.shape[0] for r in rows) < K:
            rows.append(features(sd, cfg, make_wave(2, T, s), layer).reshape(-1, cfg["hidden_size"]))
            s += 1
    allf = torch.cat(rows)
    pick = torch.randperm(allf.shape[0], generator=torch.Generator().manual_seed(seed + 7))[:K]
    return allf[pick].float().contiguous()


@functools.lru_cache(maxsize=None)
def tolerance_small(layer, T=5000):
    """(tolerance, table) at LSMALL for hidden_states[layer]: a tenth of the smallest movement among the faults that apply there
    (FAULTS_MID for layer < 4, FAULTS_END for layer == 4), and every fault's movement"""
    sd, wave = small_state_dict(), make_wave(2, T, 11)
    faults = FAULTS_END if layer == LSMALL["num_hidden_layers"] else FAULTS_MID
    with torch.no_grad():
        ref = features(sd, LSMALL, wave, layer)
        table = {f: movement(features(sd, LSMALL, wave, layer, fault=f), ref) for f in faults}
    return min(table.values()) / 10.0, table
