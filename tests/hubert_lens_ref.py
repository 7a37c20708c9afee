"""tests/hubert_ref.py restated for a padded batch with per-row sample counts: HubertWithKmeans(wave, lens=).  One batched pass in
fp64 in which every place where a row could see its padding, or its neighbours' frames past its own, is resolved about the row's own
length -- the same places include/vbx.h ("ragged waves") names for the kernels:

  * GroupNorm's statistics run over the row's own L0_b positions, and positions from L0_b on are stored as zeros;
  * the strided convolutions run as they are (no padding: a live output reads live inputs only);
  * the positional convolution sees zeros from frame N_b on, and rows from N_b on are zeros;
  * attention masks the keys from N_b on;
  * the frames from N_b on of the result are 0.0.

tests/test_hubert_lens_cpu.py holds it to hubert_ref.features of each row alone (1e-12): it is a restatement, not a second opinion.
fault=NAME plants ONE partial error (LENS_FAULTS): what a kernel does that forgets one of the places above.  The distance each moves
the live frames, with tolerance_small(), sets the tolerance of the feature tests under lengths.
"""
import torch
import torch.nn.functional as F

import hubert_ref as R

LENS_FAULTS = ("stats_padded_row", "pos_reads_past", "attn_all_keys")


def frame_lens(lens, cfg):
    return [R.frames_of(int(l), cfg) for l in lens]


def min_samples(cfg):
    n = 1
    for k, s in zip(reversed(cfg["conv_kernel"]), reversed(cfg["conv_stride"])):
        n = (n - 1) * s + k
    return n


def features_lens(sd, cfg, wave, lens, layer, emulate=False, fault=None):
    """hidden_states[layer] of the padded batch wave [B, T] under lens (ints), fp64 [B, N, D], zeros from frame N_b on"""
    assert fault is None or fault in LENS_FAULTS, fault
    e = emulate
    p = lambda n: sd[n].double()
    eps, D, H = cfg["layer_norm_eps"], cfg["hidden_size"], cfg["num_attention_heads"]
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), p(n + ".weight"), p(n + ".bias"), eps)
    k0, s0 = cfg["conv_kernel"][0], cfg["conv_stride"][0]
    B, T = wave.shape
    lens = [int(l) for l in lens]
    assert len(lens) == B and all(min_samples(cfg) <= l <= T for l in lens), lens
    x = F.conv1d(wave.double()[:, None, :], p("feature_extractor.conv_layers.0.conv.weight"), stride=s0)  # [B, C, L0]
    L0 = x.shape[2]
    l0 = torch.tensor([(l - k0) // s0 + 1 for l in lens])
    live0 = (torch.arange(L0)[None, :] < l0[:, None])[:, None, :].double()  # [B, 1, L0]
    n0 = (torch.full((B,), float(L0), dtype=torch.float64) if fault == "stats_padded_row" else l0.double())[:, None, None]
    w0 = torch.ones_like(live0) if fault == "stats_padded_row" else live0
    mean = (x * w0).sum(2, keepdim=True) / n0
    var = (((x - mean) ** 2) * w0).sum(2, keepdim=True) / n0
    gam, bet = p("feature_extractor.conv_layers.0.layer_norm.weight"), p("feature_extractor.conv_layers.0.layer_norm.bias")
    x = (x - mean) / torch.sqrt(var + eps) * gam[None, :, None] + bet[None, :, None]
    x = R.r16(F.gelu(x), e) * live0
    for i in range(1, len(cfg["conv_kernel"])):
        x = R.r16(F.gelu(F.conv1d(x, R.r16(p(f"feature_extractor.conv_layers.{i}.conv.weight"), e), stride=cfg["conv_stride"][i])), e)
    x = x.transpose(1, 2)  # [B, N, C]
    N = x.shape[1]
    nb = torch.tensor(frame_lens(lens, cfg))
    live = (torch.arange(N)[None, :] < nb[:, None])  # [B, N]
    lv = live[:, :, None].double()
    x = R.r16(ln(x, "feature_projection.layer_norm"), e) @ R.r16(p("feature_projection.projection.weight"), e).t() + p("feature_projection.projection.bias")
    k = cfg["num_conv_pos_embeddings"]
    w = R.r16(R.fold_weight_norm(sd[R.G0], sd[R.G1], e), e)
    xin = R.r16(x, e) if fault == "pos_reads_past" else R.r16(x, e) * lv
    pos = F.conv1d(xin.transpose(1, 2), w, p("encoder.pos_conv_embed.conv.bias"), padding=k // 2, groups=cfg["num_conv_pos_embedding_groups"])[..., :-1]
    x = (x + F.gelu(pos).transpose(1, 2)) * lv
    x = ln(x, "encoder.layer_norm")
    scale = (D // H) ** -0.5
    heads = lambda t: t.view(B, N, H, D // H).transpose(1, 2)
    dead_keys = torch.zeros(B, 1, 1, N, dtype=torch.float64)
    if fault != "attn_all_keys":
        dead_keys.masked_fill_(~live[:, None, None, :], float("-inf"))
    for l in range(layer):
        pre = f"encoder.layers.{l}."
        lin = lambda t, n: t @ R.r16(p(pre + n + ".weight"), e).t() + p(pre + n + ".bias")
        t16 = R.r16(x, e)
        q, kk, v = lin(t16, "attention.q_proj") * scale, lin(t16, "attention.k_proj"), lin(t16, "attention.v_proj")
        if e:
            logits = (heads(R.r16(q * R.LOG2E, e)) @ heads(R.r16(kk, e)).transpose(-1, -2)) / R.LOG2E
        else:
            logits = heads(q) @ heads(kk).transpose(-1, -2)
        o = torch.softmax(logits + dead_keys, -1) @ heads(R.r16(v, e))
        x = ln(x + lin(R.r16(o.transpose(1, 2).reshape(B, N, D), e), "attention.out_proj"), pre + "layer_norm")
        ff = lin(R.r16(F.gelu(lin(R.r16(x, e), "feed_forward.intermediate_dense")), e), "feed_forward.output_dense")
        x = ln(x + ff, pre + "final_layer_norm")
    return x * lv


def rows_alone(sd, cfg, wave, lens, layer, emulate=False):
    """[hubert_ref.features(wave[b:b+1, :len_b])[0] for every row]: fp64 [N_b, D] each"""
    return [R.features(sd, cfg, wave[b:b + 1, :int(l)], layer, emulate=emulate)[0] for b, l in enumerate(lens)]


def live_movement(got, alone):
    """max over the rows of movement(live frames of row b, the row alone)"""
    return max(R.movement(got[b, :a.shape[0]].double(), a) for b, a in enumerate(alone))


def zero_padded(wave, lens):
    w = wave.clone()
    for b, l in enumerate(lens):
        w[b, int(l):] = 0.0
    return w


LENS_CASE = dict(T=5000, lens=(5000, 3333, 1285, 719), seed=11, layer=4)


_TOL = {}


def tolerance_lens():
    """(tolerance, table) at SMALL, layer 4, on non-silent make_wave rows of 5000 samples with lengths 5000, 3333, 1285, 719:
    min(tolerance_small(), a tenth of the smallest partial fault's movement).  table: every partial fault's movement on the live
    frames against the rows alone, and "zero_padded_batch": what lens=None gives today on the zero-padded batch (all faults)."""
    if not _TOL:
        c = LENS_CASE
        sd, wave, lens = R.small_state_dict(), R.make_wave(len(c["lens"]), c["T"], c["seed"]), list(c["lens"])
        with torch.no_grad():
            alone = rows_alone(sd, R.SMALL, wave, lens, c["layer"])
            table = {f: live_movement(features_lens(sd, R.SMALL, wave, lens, c["layer"], fault=f), alone) for f in LENS_FAULTS}
            table["zero_padded_batch"] = live_movement(R.features(sd, R.SMALL, zero_padded(wave, lens), c["layer"]), alone)
        _TOL["v"] = (min(R.tolerance_small()[0], min(table[f] for f in LENS_FAULTS) / 10.0), table)
    return _TOL["v"]
