"""HubertLargeWithKmeans: the native launch sequence (csrc/hubert.hip "the large form" + vbx_gemm + vbx_attn_fwd) beside what a user
would run without it -- the same network from torch.nn.functional on the same device in fp32 and under fp16 autocast, each followed by
the same torch argmin over the codebook.  The large widths (hubert-large-ll60k's), random weights (tests/hubert_large_ref.py), 19
layers loaded, output_layer 18, K 500.  One MI355X.

    python tools/hubert_large_times.py [OUT.json]            (default: profiles/hubert_large_times.json)
    python tools/hubert_large_times.py --profile B SAMPLES    (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

The parent runs one child process per shape under `timeout -k 10 <seconds>`; a child that fails is reported and nothing is started
after it.  In a child the paths run in one process, alternating, after warm-up, device events around windows of back-to-back calls
(the host side of a call included); the minimum of the windows is the figure, the spread beside it.  The first child also times the six
normalised convolutions one by one at its shape (`--layers B SAMPLES` does only that): vbx_hubert_conv_ln (fused: the fp32 sums never
leave the LDS) beside the pair vbx_hubert_conv_f32 + vbx_hubert_ln_gelu (an fp32 intermediate plus a row kernel), together and each
alone, and which of the two vbx_hubert_conv_ln_route takes there."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 160000), (1, 16000)]
LAYERS, LAYER, K = 19, 18, 500
CALLS, REPS, WARM = 5, 5, 2


def torch_hubert_large(LR, sd, cfg, layer, dev):
    """hidden_states[layer] (layer < num_hidden_layers: no final norm) from torch's own operators on `dev` in fp32"""
    import torch.nn.functional as F

    p = {k: v.to(dev) for k, v in sd.items()}
    eps, D, H = cfg["layer_norm_eps"], cfg["hidden_size"], cfg["num_attention_heads"]
    k, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    posw = LR.fold_weight_norm(sd[LR.G0], sd[LR.G1]).float().to(dev)
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), p[n + ".weight"], p[n + ".bias"], eps)

    def fwd(wave):
        x = wave[:, None]
        for i in range(len(cfg["conv_kernel"])):
            pre = f"feature_extractor.conv_layers.{i}."
            x = F.conv1d(x, p[pre + "conv.weight"], p[pre + "conv.bias"], stride=cfg["conv_stride"][i])
            x = F.gelu(ln(x.transpose(1, 2), pre + "layer_norm").transpose(1, 2))
        x = F.linear(ln(x.transpose(1, 2), "feature_projection.layer_norm"), p["feature_projection.projection.weight"], p["feature_projection.projection.bias"])
        pos = F.conv1d(x.transpose(1, 2), posw, p["encoder.pos_conv_embed.conv.bias"], padding=k // 2, groups=G)[..., :-1]
        x = x + F.gelu(pos).transpose(1, 2)
        B, N, _ = x.shape
        heads = lambda t: t.view(B, N, H, D // H).transpose(1, 2)
        for l in range(layer):
            pre = f"encoder.layers.{l}."
            lin = lambda t, n: F.linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"])
            t = ln(x, pre + "layer_norm")
            o = F.scaled_dot_product_attention(heads(lin(t, "attention.q_proj")), heads(lin(t, "attention.k_proj")), heads(lin(t, "attention.v_proj")))
            x = x + lin(o.transpose(1, 2).reshape(B, N, D), "attention.out_proj")
            x = x + lin(F.gelu(lin(ln(x, pre + "final_layer_norm"), "feed_forward.intermediate_dense")), "feed_forward.output_dense")
        return x

    return fwd


def setup(B, T):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hubert_large_ref as LR
    import voicebox_pytorch_amd as vbx

    cfg = dict(LR.LARGE6, num_hidden_layers=LAYERS)
    sd = LR.random_state_dict(cfg, 0)
    centers = torch.randn(K, cfg["hidden_size"], generator=torch.Generator().manual_seed(1))
    model = vbx.HubertLargeWithKmeans(**cfg, output_layer=LAYER, codebook_size=K)
    model.load_state_dict(sd)
    model.set_cluster_centers(centers)
    model = model.to("cuda")
    x = LR.make_wave(B, T, 1).to("cuda")
    return torch, LR, cfg, sd, model, x


def windows(torch, paths, calls, reps):
    times = {k: [] for k in paths}
    for _ in range(reps):  # alternating windows
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return times


def summary(v, calls, reps):
    return dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=calls, windows=reps)


def conv_layers(torch, model, B, T):
    """the six normalised convolutions at this shape, one by one: the fused kernel beside the pair (see the module docstring)"""
    from voicebox_pytorch_amd import _lib

    w = model._cached(model._pack)
    C, st, eps = model.conv_dim[0], _lib.current_stream(), model.layer_norm_eps
    L = (T - model.conv_kernel[0]) // model.conv_stride[0] + 1
    out = []
    for i, kk in enumerate(model.conv_kernel[1:], 1):
        Lo = (L - kk) // 2 + 1
        a = torch.randn(B, L, C, device="cuda").half()
        y, s32 = torch.empty(B, Lo, C, dtype=torch.float16, device="cuda"), torch.empty(B, Lo, C, device="cuda")
        wc = w["convs"][i - 1]
        conv32 = lambda: _lib.call("vbx_hubert_conv_f32", a, wc, w["cb"][i], s32, B, L, C, kk, st)
        rown = lambda: _lib.call("vbx_hubert_ln_gelu", s32, w["lnw"][i], w["lnb"][i], y, B * Lo, C, eps, st)
        paths = {"fused_conv_ln": lambda: _lib.call("vbx_hubert_conv_ln", a, wc, w["cb"][i], w["lnw"][i], w["lnb"][i], y, B, L, C, kk, eps, st),
                 "pair": lambda: (conv32(), rown()), "pair_conv_f32_alone": conv32, "pair_ln_gelu_alone": rown}
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        t = {k: dict(min=min(v), max=max(v)) for k, v in windows(torch, paths, CALLS, REPS).items()}
        out.append(dict(layer=i, k=kk, L_in=L, L_out=Lo, tile_fused=_lib.call_value("vbx_hubert_conv_ln_tile", C, kk),
                        tile_pair=_lib.call_value("vbx_hubert_conv_tile", C, kk), ms=t,
                        route_taken="pair" if _lib.call_value("vbx_hubert_conv_ln_route", B, L, C, kk) else "fused"))
        L = Lo
    return out


def layers_child(B, T):
    torch, _, _, _, model, _ = setup(B, T)
    print("RESULT " + json.dumps({"B": B, "samples": T, "normalised_convolutions": conv_layers(torch, model, B, T)}))


def child(B, T, layers):
    torch, LR, cfg, sd, model, x = setup(B, T)
    ref = torch_hubert_large(LR, sd, cfg, LAYER, "cuda")
    c = model.cluster_centers
    assign = lambda h: torch.cdist(h, c[None].expand(h.shape[0], -1, -1)).argmin(-1)

    def fp32():
        with torch.inference_mode():
            return assign(ref(x))

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return assign(ref(x).float())

    paths = {"native": lambda: model(x), "torch_fp32": fp32, "torch_fp16_autocast": autocast}
    res = {"B": B, "samples": T, "frames": model.frames(T), "layers_loaded": LAYERS, "output_layer": LAYER, "codebook_size": K}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for k, v in windows(torch, paths, CALLS, REPS).items():
        res[k + "_ms_per_call"] = summary(v, CALLS, REPS)
    with torch.inference_mode():
        h32 = ref(x).double().cpu()
    res["max_over_rms_native_vs_torch_fp32"] = LR.movement(model.features(x).double().cpu(), h32)
    res["codes_native_differ_from_torch_fp32"] = float((model(x) != fp32()).float().mean())
    if layers:
        res["normalised_convolutions"] = conv_layers(torch, model, B, T)
    print("RESULT " + json.dumps(res))


def profile(B, T):
    torch, _, _, _, model, x = setup(B, T)
    for _ in range(WARM + CALLS):
        model(x)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hubert_large_times.json")
    results = {"note": f"ms per HubertLargeWithKmeans call (waves -> ids) at the large widths, {LAYERS} layers loaded, output_layer {LAYER}, K {K}, "
                       f"random weights; device events around {REPS} alternating windows of {CALLS} back-to-back calls per path in one process "
                       "(host side of the call included), one MI355X; torch_* = the same network from torch.nn.functional on the same device "
                       "(tools/hubert_large_times.py: torch_hubert_large) in fp32 and under fp16 autocast, each with torch.cdist + argmin; "
                       "normalised_convolutions: each strided convolution alone, the fused kernel beside the pair vbx_hubert_conv_f32 + "
                       "vbx_hubert_ln_gelu, min and max of the windows, and the route the module takes; produced by tools/hubert_large_times.py", "shapes": []}
    failed = False
    for i, (B, T) in enumerate(SHAPES):
        cmd = ["timeout", "-k", "10", "280", sys.executable, os.path.abspath(__file__), "--child", str(B), str(T), str(int(i == 0))]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        ok = p.returncode == 0 and line
        print(f"{B} x {T}: rc {p.returncode}", flush=True)
        results["shapes"].append(json.loads(line[0][7:]) if ok else {"B": B, "samples": T, "failed_rc": p.returncode, "stderr_tail": p.stderr[-600:]})
        if not ok:
            failed = True
            break  # nothing more is started on the device after a failure
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))
    return 1 if failed else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])))
    elif len(sys.argv) > 1 and sys.argv[1] == "--layers":
        layers_child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
