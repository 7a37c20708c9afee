"""HubertWithKmeans: the native launch sequence (csrc/hubert.hip + vbx_gemm + vbx_attn_fwd) beside what a user would run without it --
the same network from torch.nn.functional on the same device in fp32 and under fp16 autocast, and transformers.HubertModel on the
device where it imports, each followed by the same torch argmin over the codebook.  Base widths, random weights (tests/hubert_ref.py),
output_layer 9, K 500.  One MI355X.

    python tools/hubert_times.py [OUT.json]            (default: profiles/hubert_times.json)
    python tools/hubert_times.py --profile B SAMPLES    (native calls only: the program for `rocprofv3 --kernel-trace --stats --`)

The parent runs one child process per shape under `timeout -k 10 <seconds>`, then one for the train step (dim 512, depth 12,
text-conditioned over LogMelCodec: a step from 8 x 163 840-sample waves with wav2vec=tok beside the same step with the ids given); a
child that fails is reported and not run again, and nothing is started after it.  In a child the paths run in one process,
alternating, after warm-up, device events around windows of back-to-back calls (the host side of a call included); the minimum of
the windows is the figure for the tokenizer, the median of the steps for the train step, the spread beside both."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 163840), (1, 16000)]
LAYER, K = 9, 500
CALLS, REPS, WARM = 5, 5, 2
TRAIN_STEPS = 9


def torch_hubert(R, sd, cfg, layer, dev):
    """hidden_states[layer] from torch's own operators on `dev` in the dtype of the weights (fp32): tests/hubert_ref.py without fp64"""
    import torch
    import torch.nn.functional as F

    p = {k: v.to(dev) for k, v in sd.items()}
    eps, C, D, H = cfg["layer_norm_eps"], cfg["conv_dim"][0], cfg["hidden_size"], cfg["num_attention_heads"]
    k, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    posw = R.fold_weight_norm(sd[R.G0], sd[R.G1]).float().to(dev)
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), p[n + ".weight"], p[n + ".bias"], eps)

    def fwd(wave):
        x = F.conv1d(wave[:, None], p["feature_extractor.conv_layers.0.conv.weight"], stride=cfg["conv_stride"][0])
        x = F.gelu(F.group_norm(x, C, p["feature_extractor.conv_layers.0.layer_norm.weight"], p["feature_extractor.conv_layers.0.layer_norm.bias"], eps))
        for i in range(1, len(cfg["conv_kernel"])):
            x = F.gelu(F.conv1d(x, p[f"feature_extractor.conv_layers.{i}.conv.weight"], stride=cfg["conv_stride"][i]))
        x = F.linear(ln(x.transpose(1, 2), "feature_projection.layer_norm"), p["feature_projection.projection.weight"], p["feature_projection.projection.bias"])
        pos = F.conv1d(x.transpose(1, 2), posw, p["encoder.pos_conv_embed.conv.bias"], padding=k // 2, groups=G)[..., :-1]
        x = ln(x + F.gelu(pos).transpose(1, 2), "encoder.layer_norm")
        B, N, _ = x.shape
        heads = lambda t: t.view(B, N, H, D // H).transpose(1, 2)
        for l in range(layer):
            pre = f"encoder.layers.{l}."
            lin = lambda t, n: F.linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"])
            o = F.scaled_dot_product_attention(heads(lin(x, "attention.q_proj")), heads(lin(x, "attention.k_proj")), heads(lin(x, "attention.v_proj")))
            x = ln(x + lin(o.transpose(1, 2).reshape(B, N, D), "attention.out_proj"), pre + "layer_norm")
            x = ln(x + lin(F.gelu(lin(x, "feed_forward.intermediate_dense")), "feed_forward.output_dense"), pre + "final_layer_norm")
        return x

    return fwd


def setup(B, T):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hubert_ref as R
    import voicebox_pytorch_amd as vbx

    sd = R.base_state_dict()
    centers = torch.randn(K, R.BASE["hidden_size"], generator=torch.Generator().manual_seed(1))
    model = vbx.HubertWithKmeans(**R.BASE, output_layer=LAYER, codebook_size=K)
    model.load_state_dict(sd)
    model.set_cluster_centers(centers)
    model = model.to("cuda")
    x = R.make_wave(B, T, 1).to("cuda")
    return torch, R, sd, model, x


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


def child(B, T):
    torch, R, sd, model, x = setup(B, T)
    ref = torch_hubert(R, sd, R.BASE, LAYER, "cuda")
    c = model.cluster_centers
    assign = lambda h: torch.cdist(h, c[None].expand(h.shape[0], -1, -1)).argmin(-1)

    def fp32():
        with torch.inference_mode():
            return assign(ref(x))

    def autocast():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return assign(ref(x).float())

    paths = {"native": lambda: model(x), "torch_fp32": fp32, "torch_fp16_autocast": autocast}
    try:
        import transformers

        hc = transformers.HubertConfig(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in R.BASE.items()}, hidden_dropout=0.0,
                                       attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)
        hf = transformers.HubertModel(hc)
        hf.load_state_dict(sd, strict=False)
        hf = hf.to("cuda").eval()

        def library():
            with torch.inference_mode():
                return assign(hf(x, output_hidden_states=True).hidden_states[LAYER])

        paths["transformers_fp32_all_12_layers"] = library
    except Exception as e:  # the library is an optional arm
        print("transformers arm left out:", type(e).__name__, e, file=sys.stderr)
    res = {"B": B, "samples": T, "frames": model.frames(T), "output_layer": LAYER, "codebook_size": K}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for k, v in windows(torch, paths, CALLS, REPS).items():
        res[k + "_ms_per_call"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), calls=CALLS, windows=REPS)
    with torch.inference_mode():
        h32 = ref(x).double().cpu()
    res["max_over_rms_native_vs_torch_fp32"] = R.movement(model.features(x).double().cpu(), h32)
    res["codes_native_differ_from_torch_fp32"] = float((model(x) != fp32()).float().mean())
    print("RESULT " + json.dumps(res))


def train_child(B, T):
    torch, R, sd, tok, _ = setup(1, 400)
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.dp import TrainStep

    wave = R.make_wave(B, T, 2, rate=24000).to("cuda")
    torch.manual_seed(0)
    kw = dict(dim=512, num_cond_tokens=K, depth=12, dim_head=64, heads=8, condition_on_text=True)
    vb = vbx.VoiceBox(audio_enc_dec=vbx.LogMelCodec(), **kw).to("cuda")
    ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb, wav2vec=tok), lr=3e-4, max_grad_norm=0.5)
    ids = tok(vbx.resample(wave, 24000, 16000))
    paths = {"step_wav2vec": lambda: ts.step(wave), "step_ids_given": lambda: ts.step(wave, cond_token_ids=ids)}
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    res = {"B": B, "samples_24k": T, "semantic_frames": ids.shape[1], "dim": 512, "depth": 12}
    for k, v in windows(torch, paths, 1, TRAIN_STEPS).items():
        res[k + "_ms"] = dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), steps=TRAIN_STEPS)
    res["wav2vec_share_of_step_median"] = 1.0 - res["step_ids_given_ms"]["median"] / res["step_wav2vec_ms"]["median"]
    print("RESULT " + json.dumps(res))


def profile(B, T):
    torch, _, _, model, x = setup(B, T)
    for _ in range(WARM + CALLS):
        model(x)
    torch.cuda.synchronize()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hubert_times.json")
    results = {"note": f"ms per HubertWithKmeans call (waves -> ids) at the base widths, output_layer {LAYER}, K {K}, random weights; device "
                       f"events around {REPS} alternating windows of {CALLS} back-to-back calls per path in one process (host side of the call "
                       "included), one MI355X; torch_* = the same network from torch.nn.functional on the same device (tools/hubert_times.py: "
                       "torch_hubert) in fp32 and under fp16 autocast, transformers_* = transformers.HubertModel (fp32, which runs all 12 "
                       "layers), each with torch.cdist + argmin; train_step: dim 512 / depth 12 text-conditioned over LogMelCodec, medians of "
                       "alternating single steps; produced by tools/hubert_times.py", "shapes": []}
    jobs = [("--child", B, T, "shapes") for B, T in SHAPES] + [("--train-child", SHAPES[0][0], SHAPES[0][1], "train_step")]
    failed = False
    for mode, B, T, key in jobs:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), mode, str(B), str(T)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        ok = p.returncode == 0 and line
        entry = json.loads(line[0][7:]) if ok else {"B": B, "samples": T, "failed_rc": p.returncode, "stderr_tail": p.stderr[-600:]}
        if key == "shapes":
            results["shapes"].append(entry)
        else:
            results[key] = entry
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
        child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--train-child":
        train_child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
