"""HuBERT base (feat_extract_norm="group", post-LN encoder, no convolution bias) restated in fp64 from F.conv1d / F.group_norm /
F.layer_norm / F.gelu / softmax, with transformers.HubertModel's parameter names -- the yardstick of voicebox_pytorch_amd.HubertWithKmeans.
tests/test_hubert_cpu.py holds it against the library itself (1e-10 at every hidden state), so unlike the codec restatements this one
is PINNED.  Self-contained: the GPU tests import nothing else.

emulate=True rounds operands and stored activations to fp16 exactly where include/vbx.h ("HuBERT + k-means") says the kernels do, and
nowhere else; all sums stay fp64.  What it does not mirror: fp32 summation order, the fp16 probabilities inside vbx_attn_fwd and the
Abramowitz-Stegun erf of VBX_EPI_GELU.

fault=NAME plants one deliberate error (FAULTS): the distance each moves the features sets the tolerance of the feature tests.
"""
import functools
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634

SMALL = dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, intermediate_size=512, conv_dim=(32,) * 7,
             conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16,
             num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5)
BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, conv_dim=(512,) * 7,
            conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=128,
            num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5)

# structural faults: each is a different network.  The feature tolerance is a tenth of the smallest movement among THESE.
FAULTS = ("gn_over_channels", "pos_first_dropped", "pos_pad_k2m1", "wn_per_out_channel", "q_scale_before_bias", "pre_ln",
          "no_encoder_ln", "prev_hidden")
# approximation-level perturbations, reported beside them but not part of the minimum: tanh-GELU differs from erf-GELU by at most
# 4.8e-4 absolute and the unbiased variance by a factor 1 + 1 / (2 (L0 - 1)) on rstd, which vanishes with the length of the wave --
# both lie below what fp16 operands (2^-11 relative per rounding) resolve, so no fp16 kernel could be told from them.
SOFT_FAULTS = ("tanh_gelu", "unbiased_var")

G0, G1 = "encoder.pos_conv_embed.conv.parametrizations.weight.original0", "encoder.pos_conv_embed.conv.parametrizations.weight.original1"


def frames_of(T, cfg):
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        T = (T - k) // s + 1
    return T


def random_state_dict(cfg, seed, dtype=torch.float32):
    """Parameters under transformers.HubertModel's names.  Not the library's initialisation (its biases are zero and its linear
    weights 0.02: half the FAULTS would move nothing): unit-gain weights, biases of std 0.3, norm gains around one, weight-norm gains
    that make the positional embedding as large as its input.  The two residual branches end at HALF gain (out_proj, output_dense): at
    unit gain the common part every frame gets from a random branch grows under each LayerNorm and the frames bunch -- their spread
    about the mean frame shrinks by 0.65 per layer, to 2 % of the RMS at layer 9 of the base widths, where no codebook can tell them
    apart; at half gain 20 % is left."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    D, I, C, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["conv_dim"][0], cfg["num_hidden_layers"]
    k, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    sd = {}
    cin = 1
    for i, kk in enumerate(cfg["conv_kernel"]):
        sd[f"feature_extractor.conv_layers.{i}.conv.weight"] = rn(C, cin, kk) * math.sqrt(2.0 / (cin * kk))
        cin = C
    norm = lambda n, p: sd.update({p + ".weight": 0.75 + 0.5 * ru(n), p + ".bias": 0.2 * rn(n)})
    lin = lambda o, i_, p, gain=1.0: sd.update({p + ".weight": gain * rn(o, i_) / math.sqrt(i_), p + ".bias": gain * 0.3 * rn(o)})
    norm(C, "feature_extractor.conv_layers.0.layer_norm")
    norm(C, "feature_projection.layer_norm")
    lin(D, C, "feature_projection.projection")
    sd["encoder.pos_conv_embed.conv.bias"] = 0.3 * rn(D)
    sd[G0] = (0.5 + ru(1, 1, k)) * math.sqrt(D / k)
    sd[G1] = rn(D, D // G, k)
    norm(D, "encoder.layer_norm")
    for l in range(L):
        p = f"encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj"):
            lin(D, D, p + "attention." + n)
        lin(D, D, p + "attention.out_proj", 0.5)
        norm(D, p + "layer_norm")
        lin(I, D, p + "feed_forward.intermediate_dense")
        lin(D, I, p + "feed_forward.output_dense", 0.5)
        norm(D, p + "final_layer_norm")
    return {k_: v.to(dtype) for k_, v in sd.items()}


def make_wave(B, T, seed, rate=16000):
    """noise plus a chirp under a slow envelope (pure white noise through a random network bunches the frames), fp32 [B, T]"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64) / rate
    rows = []
    for _ in range(B):
        f0, f1, ph, fe = (float(v) for v in torch.rand(4, generator=g, dtype=torch.float64))
        chirp = torch.sin(2 * math.pi * ((100 + 300 * f0) * t + (400 + 1600 * f1) * t * t / max(T / rate, 1e-3) / 2) + 6.28 * ph)
        env = 0.55 + 0.45 * torch.sin(2 * math.pi * (2 + 3 * fe) * t + 6.28 * f0)
        rows.append(env * (0.6 * chirp + 0.25 * torch.randn(T, generator=g, dtype=torch.float64)))
    return torch.stack(rows).float()


def r16(t, on):
    return t.half().double() if on else t


def fold_weight_norm(g, v, emulate=False, per_out_channel=False):
    """weight norm at dim=2: one norm per tap over (out, in).  The device module folds in fp32; emulate does the same."""
    dt = torch.float32 if emulate else torch.float64
    g, v = g.to(dt), v.to(dt)
    if per_out_channel:  # the fault: nn.utils.weight_norm's default dim=0, the k gains dealt to the output channels in turn
        gg = g.flatten()[torch.arange(v.shape[0]) % g.numel()].view(-1, 1, 1)
        return (v * (gg / v.norm(dim=(1, 2), keepdim=True))).double()
    return (v * (g / v.norm(dim=(0, 1), keepdim=True))).double()


def hidden_states(sd, cfg, wave, upto=None, emulate=False, fault=None):
    """[hidden_states[0], ..., hidden_states[upto]] as transformers.HubertModel(output_hidden_states=True) names them, fp64 [B, N, D]"""
    assert fault is None or fault in FAULTS + SOFT_FAULTS, fault
    e = emulate
    p = lambda n: sd[n].double()
    eps, C, D, H = cfg["layer_norm_eps"], cfg["conv_dim"][0], cfg["hidden_size"], cfg["num_attention_heads"]
    L = cfg["num_hidden_layers"] if upto is None else upto
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if fault == "tanh_gelu" else F.gelu
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), p(n + ".weight"), p(n + ".bias"), eps)
    x = F.conv1d(wave.double()[:, None, :], p("feature_extractor.conv_layers.0.conv.weight"), stride=cfg["conv_stride"][0])
    gam, bet = p("feature_extractor.conv_layers.0.layer_norm.weight"), p("feature_extractor.conv_layers.0.layer_norm.bias")
    if fault == "gn_over_channels":
        x = F.layer_norm(x.transpose(1, 2), (C,), None, None, eps).transpose(1, 2) * gam[:, None] + bet[:, None]
    elif fault == "unbiased_var":
        x = (x - x.mean(2, keepdim=True)) / torch.sqrt(x.var(2, unbiased=True, keepdim=True) + eps) * gam[:, None] + bet[:, None]
    else:
        x = F.group_norm(x, C, gam, bet, eps)
    x = r16(gelu(x), e)
    for i in range(1, len(cfg["conv_kernel"])):
        x = r16(gelu(F.conv1d(x, r16(p(f"feature_extractor.conv_layers.{i}.conv.weight"), e), stride=cfg["conv_stride"][i])), e)
    x = x.transpose(1, 2)
    x = r16(ln(x, "feature_projection.layer_norm"), e) @ r16(p("feature_projection.projection.weight"), e).t() + p("feature_projection.projection.bias")
    k = cfg["num_conv_pos_embeddings"]
    w = r16(fold_weight_norm(sd[G0], sd[G1], e, per_out_channel=fault == "wn_per_out_channel"), e)
    xin = r16(x, e).transpose(1, 2)
    if fault == "pos_pad_k2m1":
        pos = F.conv1d(F.pad(xin, (k // 2 - 1, k // 2)), w, p("encoder.pos_conv_embed.conv.bias"), groups=cfg["num_conv_pos_embedding_groups"])
    else:
        pos = F.conv1d(xin, w, p("encoder.pos_conv_embed.conv.bias"), padding=k // 2, groups=cfg["num_conv_pos_embedding_groups"])
        pos = pos[..., 1:] if fault == "pos_first_dropped" else pos[..., :-1]
    x = x + gelu(pos).transpose(1, 2)
    if fault != "no_encoder_ln":
        x = ln(x, "encoder.layer_norm")
    hs = [x]
    scale = (D // H) ** -0.5
    B, N, _ = x.shape
    heads = lambda t: t.view(B, N, H, D // H).transpose(1, 2)
    for l in range(L):
        pre = f"encoder.layers.{l}."
        lin = lambda t, n: t @ r16(p(pre + n + ".weight"), e).t() + p(pre + n + ".bias")

        def attn(t):
            t16 = r16(t, e)
            if fault == "q_scale_before_bias":
                q = (t16 @ r16(p(pre + "attention.q_proj.weight"), e).t()) * scale + p(pre + "attention.q_proj.bias")
            else:
                q = lin(t16, "attention.q_proj") * scale
            kk, v = lin(t16, "attention.k_proj"), lin(t16, "attention.v_proj")
            if e:  # q16 = fp16(q * scale * log2(e)), the attention kernels' contract: q16 . k16 is the exponent of exp2
                logits = (heads(r16(q * LOG2E, e)) @ heads(r16(kk, e)).transpose(-1, -2)) / LOG2E
            else:
                logits = heads(q) @ heads(kk).transpose(-1, -2)
            o = torch.softmax(logits, -1) @ heads(r16(v, e))
            return lin(r16(o.transpose(1, 2).reshape(B, N, D), e), "attention.out_proj")

        ff = lambda t: lin(r16(gelu(lin(r16(t, e), "feed_forward.intermediate_dense")), e), "feed_forward.output_dense")
        if fault == "pre_ln":
            x = x + attn(ln(x, pre + "layer_norm"))
            x = x + ff(ln(x, pre + "final_layer_norm"))
        else:
            x = ln(x + attn(x), pre + "layer_norm")
            x = ln(x + ff(x), pre + "final_layer_norm")
        hs.append(x)
    return hs


def features(sd, cfg, wave, layer, emulate=False, fault=None):
    """hidden_states[layer], fp64 [B, N, D]; the fault "prev_hidden" answers with hidden_states[layer - 1]"""
    hs = hidden_states(sd, cfg, wave, upto=layer, emulate=emulate, fault=fault)
    return hs[layer - 1] if fault == "prev_hidden" else hs[layer]


def kmeans_assign(h, centers):
    """the Euclidean argmin in fp64 (lowest index on a tie) and the distances [.., K]"""
    d = ((h.double()[..., None, :] - centers.double()) ** 2).sum(-1)
    return d.argmin(-1), d


def kmeans_bound(h, centers):
    """the slack of vbx_kmeans_assign's contract per frame: (D + 2) * 2^-23 * (|h| + max |c|)^2"""
    D = h.shape[-1]
    return (D + 2) * 2.0 ** -23 * (h.double().norm(dim=-1) + centers.double().norm(dim=-1).max()) ** 2


def movement(a, b):
    """max |a - b| over the RMS of b: the measure of the feature tolerance"""
    return float((a - b).abs().max() / b.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _cached_sd(name, seed):
    return random_state_dict(dict(SMALL=SMALL, BASE=BASE)[name], seed)


def small_state_dict(seed=0):
    return _cached_sd("SMALL", seed)


def base_state_dict(seed=0):
    return _cached_sd("BASE", seed)


@functools.lru_cache(maxsize=None)
def codebook(name, seed, layer, K, frames_per_wave=99):
    """K feature frames of OTHER waves through the same network (fp64 restatement), fp32 [K, D]: codes as a k-means of such
    features would place them, not random points far from every frame"""
    cfg = dict(SMALL=SMALL, BASE=BASE)[name]
    sd = _cached_sd(name, seed)
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
def tolerance_small(layer=4, T=5000):
    """(tolerance, table): a tenth of the smallest structural fault's movement at SMALL, and every fault's movement"""
    sd, wave = small_state_dict(), make_wave(2, T, 11)
    with torch.no_grad():
        ref = features(sd, SMALL, wave, layer)
        table = {f: movement(features(sd, SMALL, wave, layer, fault=f), ref) for f in FAULTS + SOFT_FAULTS}
    return min(table[f] for f in FAULTS) / 10.0, table
