"""Times of the codec-latent kernels and steps on one MI355X (device events, 5 windows of back-to-back calls each):
    python tools/codec_times.py [OUT.json]        (default: codec_times.json in the current directory)"""
import json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import voicebox_pytorch_amd as vbx
from voicebox_pytorch_amd import _lib as L
from toy_codec import ToyCodec

dev = "cuda"
def window(fn, calls=50, reps=5, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls): fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return dict(min_ms=min(out), max_ms=max(out), median_ms=sorted(out)[len(out) // 2], calls=calls, repeats=reps)

res = {}
codec = vbx.LogMelCodec().to(dev)
wave = torch.randn(8, 163840, device=dev)
res["logmel_encode_8x163840"] = window(lambda: codec.encode(wave))
st = lambda: torch.cuda.current_stream().cuda_stream
B, N, Lc, D = 8, 1024, 100, 512
Kp = L.lib().vbx_proj_in_kp(Lc)
x, cond = torch.randn(B, N, Lc, device=dev), torch.randn(B, N, Lc, device=dev)
wh = torch.zeros(D, Kp, dtype=torch.float16, device=dev); wh[:, :Lc] = torch.randn(D, Lc, device=dev) * 0.1
bias = torch.randn(D, device=dev)
cm = (torch.rand(B, N, device=dev) < 0.8).view(torch.uint8)
o16 = torch.empty(B * N, 2 * D, dtype=torch.float16, device=dev); ob = torch.empty_like(o16).view(torch.bfloat16)
xcb = torch.empty(2 * B * N, Kp, dtype=torch.bfloat16, device=dev)
res["proj_in_embed_fwd_train_dim512_L100_8x1024"] = window(lambda: L.call("vbx_proj_in_embed", x, cond, wh, bias, cm, None, None, o16, ob, xcb, B, N, Lc, D, 0, st()))
res["proj_in_embed_fwd_infer_dim512_L100_8x1024"] = window(lambda: L.call("vbx_proj_in_embed", x, cond, wh, bias, cm, None, None, o16, None, None, B, N, Lc, D, 0, st()))
# the backward stages added for proj_in: d(x') / d(cond') through to_embed (two NN products), the split-K weight gradient over the packed
# [2M, Kp] operand, its reduce
import ctypes as C
M = B * N
deb = torch.randn(M, D, device=dev).to(torch.bfloat16)
embb = (torch.randn(D, 2 * D, device=dev) * 0.05).to(torch.bfloat16)
dxc = torch.empty(2 * M, D, dtype=torch.bfloat16, device=dev)
splits = 8
slabs = torch.empty(splits, D, Kp, device=dev)
dw, db = torch.empty(D, Lc, device=dev), torch.empty(D, device=dev)
def desc(mode, epi, m, n, k, lda, ldb, ldc, a, b, c, sp=0):
    g = L.GemmDesc()
    g.mode, g.epilogue, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.splits = mode, epi, m, n, k, lda, ldb, ldc, sp
    g.A, g.B, g.C = a, b, c
    return g
g1 = desc(L.VBX_GEMM_NN, L.VBX_EPI_BF16, M, D, D, D, 2 * D, D, deb.data_ptr(), embb.data_ptr(), dxc.data_ptr())
g2 = desc(L.VBX_GEMM_NN, L.VBX_EPI_BF16, M, D, D, D, 2 * D, D, deb.data_ptr(), embb.data_ptr() + 2 * D, dxc.data_ptr() + 2 * M * D)
g3 = desc(L.VBX_GEMM_TN, L.VBX_EPI_SPLITK, D, Kp, 2 * M, D, Kp, 0, dxc.data_ptr(), xcb.data_ptr(), slabs.data_ptr(), splits)
def bwd():
    L.call("vbx_gemm", C.byref(g1), st()); L.call("vbx_gemm", C.byref(g2), st()); L.call("vbx_gemm", C.byref(g3), st())
    L.call("vbx_proj_in_wgrad_reduce", slabs, splits, D, Lc, dw, db, st())
res["proj_in_backward_stages_dim512_L100_8x1024_8_splits"] = window(bwd)
# whole train step of a dim-512 / depth-12 model: codec-latent (L = 100 into 512, waves in) beside dim_in = 104 (no proj_in) as the nearest existing path
from voicebox_pytorch_amd.dp import TrainStep
def step_time(vb, inp):
    vb = vb.to(dev)
    ts = TrainStep(vbx.ConditionalFlowMatcherWrapper(voicebox=vb), lr=1e-4, max_grad_norm=0.5)
    r = window(lambda: ts.step(inp), calls=10, reps=5, warm=5)
    del ts, vb
    torch.cuda.empty_cache()
    return r
kw = dict(dim=512, depth=12, heads=16, dim_head=64, num_cond_tokens=500, condition_on_text=False)
torch.manual_seed(0)
lat = torch.randn(8, 1024, 100, device=dev)
res["train_step_codec_L100_dim512_depth12_8x1024_from_latents"] = step_time(vbx.VoiceBox(audio_enc_dec=ToyCodec(100), **kw), lat)
res["train_step_codec_L100_dim512_depth12_8x1024_from_waves_toy_codec"] = step_time(vbx.VoiceBox(audio_enc_dec=ToyCodec(100), **kw), torch.randn(8, 1024 * 16, device=dev))
res["train_step_logmel_dim512_depth12_8x1024_from_waves"] = step_time(vbx.VoiceBox(audio_enc_dec=vbx.LogMelCodec(), **kw), torch.randn(8, 1023 * 160, device=dev))
res["train_step_dim_in104_dim512_depth12_8x1024"] = step_time(vbx.VoiceBox(dim_in=104, **kw), torch.randn(8, 1024, 104, device=dev))
res["train_step_codec_free_dim512_depth12_8x1024"] = step_time(vbx.VoiceBox(**kw), torch.randn(8, 1024, 512, device=dev))
OUT = sys.argv[1] if len(sys.argv) > 1 else "codec_times.json"
json.dump(res, open(OUT, "w"), indent=1)
print(json.dumps(res, indent=1))
