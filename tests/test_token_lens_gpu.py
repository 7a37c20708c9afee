"""Per-row token resize (vbx_io.tok_lens; token_lens= / cond_token_lens=) and wave_lens= with token ids from wav2vec=.

Kernels: vbx_pack_embed_input_text_lens and vbx_embed_text_cols_lens against the PLAIN entries on each row alone (B = 1, N = N_b,
T = T_b) bit for bit on the live rows, cond_emb zero on the dead ones; vbx_cond_emb_bwd_lens against an fp64 scatter through the same
resize weights, with the tolerance tests/test_ops_gpu.py holds vbx_cond_emb_bwd to (fp32 atomics: no bit claim).
Model: wrapper(waves, wave_lens=) with wav2vec=HubertWithKmeans IS wrapper(latents, lens=F, semantic_token_ids=ids, token_lens=TL)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import hubert_ref as R
from attn_check import rel_err

pytestmark = pytest.mark.gpu
dev = "cuda"


def st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    return _lib


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _u8(t):
    return None if t is None else t.to(torch.uint8).to(dev)


ROWS = {"ragged": [(13, 24), (7, 15), (1, 1)], "identity": [(13, 13), (5, 5), (1, 7)]}


# ----------------------------------------------------------------------------- the three *_lens embed entries
@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("dropped", [None, 1])
def test_embed_lens_entries_are_the_rows_alone(L, rows, dropped):
    Bsz, N, T, E, D, V = 3, 24, 13, 16, 16, 50
    pairs = ROWS[rows]
    g = _gen(len(rows) + (dropped or 0))
    x, cond = torch.randn(Bsz, N, D, generator=g), torch.randn(Bsz, N, D, generator=g)
    cmask = torch.rand(Bsz, N, generator=g) < 0.4
    drop = None if dropped is None else torch.tensor([b == dropped for b in range(Bsz)])
    null_cond = torch.randn(D, generator=g)
    ids = torch.randint(0, V, (Bsz, T), generator=g)
    table = torch.randn(V + 1, E, generator=g)
    xd, cd, cm, nc, idd, tb = x.to(dev), cond.to(dev), _u8(cmask), null_cond.to(dev), ids.to(dev), table.to(dev)
    tok, frames = _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
    W = 2 * D + E

    def pack_lens(tok, key, Rr):
        o16 = torch.full((Bsz * N, W), float("nan"), dtype=torch.float16, device=dev)
        ob = torch.full((Bsz * N, W), float("nan"), dtype=torch.bfloat16, device=dev)
        L.call("vbx_pack_embed_input_text_lens", xd, cd, cm, _u8(drop), nc, idd, T, tok, key, Rr, tb, E, V, o16, ob, Bsz, N, D, st())
        return o16.cpu().view(Bsz, N, W), ob.cpu().view(Bsz, N, W)

    o16, ob = pack_lens(tok, frames, 0)
    # the plain entry on the whole batch: what the x and cond' columns hold on every row, dead ones included
    p16, pb = torch.empty(Bsz * N, W, dtype=torch.float16, device=dev), torch.empty(Bsz * N, W, dtype=torch.bfloat16, device=dev)
    L.call("vbx_pack_embed_input_text", xd, cd, cm, _u8(drop), nc, idd, T, tb, E, V, p16, pb, Bsz, N, D, st())
    p16, pb = p16.cpu().view(Bsz, N, W), pb.cpu().view(Bsz, N, W)
    ld, col0 = W + 8, D
    c16 = torch.full((Bsz * N, ld), 7.0, dtype=torch.float16, device=dev)
    cb = torch.full((Bsz * N, ld), 7.0, dtype=torch.bfloat16, device=dev)
    L.call("vbx_embed_text_cols_lens", _u8(drop), idd, T, tok, frames, 0, tb, E, V, c16, cb, Bsz, N, col0, ld, st())
    c16, cb = c16.cpu().view(Bsz, N, ld), cb.cpu().view(Bsz, N, ld)
    for b, (Tb, Nb) in enumerate(pairs):
        xa, ca = x[b:b + 1, :Nb].contiguous().to(dev), cond[b:b + 1, :Nb].contiguous().to(dev)
        da = None if drop is None else _u8(drop[b:b + 1])
        ia = ids[b:b + 1, :Tb].contiguous().to(dev)
        a16, ab = torch.empty(Nb, W, dtype=torch.float16, device=dev), torch.empty(Nb, W, dtype=torch.bfloat16, device=dev)
        L.call("vbx_pack_embed_input_text", xa, ca, _u8(cmask[b:b + 1, :Nb].contiguous()), da, nc, ia, Tb, tb, E, V, a16, ab, 1, Nb, D, st())
        assert torch.equal(o16[b, :Nb], a16.cpu()) and torch.equal(ob[b, :Nb], ab.cpu()), (rows, b)
        assert (o16[b, Nb:, D:D + E].view(torch.int16) == 0).all() and (ob[b, Nb:, D:D + E].view(torch.int16) == 0).all()
        for lo, hi in ((0, D), (D + E, W)):  # x and cond' are written as ever
            assert torch.equal(o16[b, :, lo:hi], p16[b, :, lo:hi]) and torch.equal(ob[b, :, lo:hi], pb[b, :, lo:hi])
        e16, eb = torch.full((Nb, ld), 7.0, dtype=torch.float16, device=dev), torch.full((Nb, ld), 7.0, dtype=torch.bfloat16, device=dev)
        L.call("vbx_embed_text_cols", da, ia, Tb, tb, E, V, e16, eb, 1, Nb, col0, ld, st())
        assert torch.equal(c16[b, :Nb], e16.cpu()) and torch.equal(cb[b, :Nb], eb.cpu()), (rows, b)
        assert torch.equal(c16[b, :Nb, col0:col0 + E], o16[b, :Nb, D:D + E])  # the two forwards agree with each other
        assert (c16[b, Nb:, col0:col0 + E].view(torch.int16) == 0).all() and (cb[b, Nb:, col0:col0 + E].view(torch.int16) == 0).all()
        assert (c16[b, :, :col0] == 7).all() and (c16[b, :, col0 + E:] == 7).all()  # nothing outside the columns is touched
    # key_lens counts R register rows in front of the frames
    r16, rb = pack_lens(tok, frames + 4, 4)
    assert torch.equal(r16, o16) and torch.equal(rb, ob)
    # tables outside their ranges are clamped on the device into 1 .. T and 1 .. N: no value becomes an index
    w16, _ = pack_lens(_i32([0, -9, 2 ** 31 - 1]), _i32([-3, 2 ** 31 - 1, 0]), 0)
    k16, _ = pack_lens(_i32([1, 1, T]), _i32([1, N, 1]), 0)
    assert torch.equal(w16.view(torch.int16), k16.view(torch.int16)) and torch.isfinite(w16.float()).all()
    # ---- the backward: an fp64 scatter through the same resize weights
    demb = torch.randn(Bsz * N, E, generator=g).to(torch.bfloat16)
    gt = torch.zeros(V + 1, E, device=dev)
    L.call("vbx_cond_emb_bwd_lens", demb.to(dev), E, idd, T, tok, frames, 0, _u8(drop), V, gt, Bsz, N, E, st())
    tab = table.double().requires_grad_(True)
    total = 0.0
    for b, (Tb, Nb) in enumerate(pairs):
        idb = torch.full((Tb,), V) if (drop is not None and bool(drop[b])) else ids[b, :Tb]
        emb = tab[idb][None]  # [1, Tb, E]
        if Tb != Nb:
            emb = F.interpolate(emb.transpose(1, 2)[..., None], (Nb, 1), mode="bilinear")[..., 0].transpose(1, 2)
        total = total + (emb[0] * demb.view(Bsz, N, E)[b, :Nb].double()).sum()  # frames past N_b add nothing
    total.backward()
    assert rel_err(gt, tab.grad) < 1e-5, rel_err(gt, tab.grad)
    gt4 = torch.zeros(V + 1, E, device=dev)
    L.call("vbx_cond_emb_bwd_lens", demb.to(dev), E, idd, T, tok, frames + 4, 4, _u8(drop), V, gt4, Bsz, N, E, st())
    assert rel_err(gt4, tab.grad) < 1e-5


def test_embed_lens_entries_refuse_missing_tables(L):
    lib = L.lib()
    z = torch.zeros(64, device=dev)
    ids = torch.zeros(4, dtype=torch.int64, device=dev)
    o = torch.zeros(64, dtype=torch.float16, device=dev)
    t = _i32([1])
    a = [P.data_ptr() if P is not None else None for P in (z, z, None, None, None, ids)]
    assert lib.vbx_pack_embed_input_text_lens(*a, 4, None, t.data_ptr(), 0, z.data_ptr(), 8, 0, o.data_ptr(), None, 1, 1, 8, st()) == -1
    assert lib.vbx_pack_embed_input_text_lens(*a, 4, t.data_ptr(), None, 0, z.data_ptr(), 8, 0, o.data_ptr(), None, 1, 1, 8, st()) == -1
    assert lib.vbx_embed_text_cols_lens(None, ids.data_ptr(), 4, None, t.data_ptr(), 0, z.data_ptr(), 8, 0, o.data_ptr(), None, 1, 1, 0, 8, st()) == -1
    assert lib.vbx_cond_emb_bwd_lens(o.data_ptr(), 8, ids.data_ptr(), 4, t.data_ptr(), None, 0, None, 0, z.data_ptr(), 1, 1, 8, st()) == -1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the model
VB_KW = dict(dim=128, num_cond_tokens=64, depth=2, dim_head=64, heads=2, condition_on_text=True, time_hidden_dim=128, ff_mult=2)
WAVE_LENS = [9600, 6001, 2000]  # at 24 kHz, LogMelCodec's rate: 61 / 38 / 13 latent frames, 19 / 12 / 3 semantic frames


@functools.lru_cache(maxsize=None)
def _tok():
    import voicebox_pytorch_amd as vbx

    centers = R.codebook("SMALL", 0, 4, 64)
    m = vbx.HubertWithKmeans(**R.SMALL, output_layer=4, codebook_size=64)
    m.load_state_dict(R.small_state_dict())
    m.set_cluster_centers(centers)
    return m.to(dev)


def _wrapper(state=None, **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(audio_enc_dec=vbx.LogMelCodec(), **VB_KW)
    if state is not None:
        vb.load_state_dict(state)
    return vbx.ConditionalFlowMatcherWrapper(voicebox=vb.to(dev), **kw)


def _draws(shape, seed=5):
    g = _gen(seed)
    return dict(x0=torch.randn(shape, generator=g), times=torch.rand(shape[0], generator=g), frac_lengths=torch.tensor([0.8, 0.9, 0.75]),
                rand=torch.rand(shape[0], generator=g))


@functools.lru_cache(maxsize=None)
def _pair():
    """two wrappers with the same weights (one with wav2vec=), the waves, and the ids / lengths the second form is called with"""
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(3)
    tok = _tok()
    w_tok = _wrapper(wav2vec=tok)
    start = {k: v.detach().cpu().clone() for k, v in w_tok.voicebox.state_dict().items()}
    wave = R.make_wave(3, 9600, 8, rate=24000).to(dev)
    wl16 = vbx.resample_lens(WAVE_LENS, 24000, 16000)
    ids = tok(vbx.resample(wave, 24000, 16000, lens=WAVE_LENS), lens=wl16)
    TL = tok.frame_lens(wl16)
    assert ids.shape == (3, 19) and TL == [19, 12, 3] and len(ids.unique()) > 4
    return w_tok, start, wave, ids, TL


def test_wrapper_wave_lens_with_wav2vec_is_the_call_with_ids_and_token_lens():
    from voicebox_pytorch_amd.masks import rng_override

    w_tok, start, wave, ids, TL = _pair()
    w_tok.voicebox.load_state_dict(start)
    w_ids = _wrapper(state=start)
    got_ids, got_tl = w_tok.wav2vec_token_ids(wave, None, wave_lens=WAVE_LENS)
    assert torch.equal(got_ids, ids) and got_tl == TL
    lat, _, FL = w_ids.encode_raw_audio(wave, None, None, wave_lens=WAVE_LENS)
    assert FL == [61, 38, 13] and lat.shape == (3, 61, 100)
    draws = _draws((3, 61, 100))
    grads = []
    for run in (lambda: w_tok(wave, wave_lens=WAVE_LENS),
                lambda: w_ids(lat, lens=FL, semantic_token_ids=ids, token_lens=TL),
                lambda: w_ids(wave, wave_lens=WAVE_LENS, semantic_token_ids=ids, token_lens=torch.tensor(TL, device=dev))):
        with rng_override(**draws):
            loss = run()
        w = w_tok if not grads else w_ids
        w.voicebox.zero_grad(set_to_none=True)
        loss.backward()
        grads.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in w.voicebox.named_parameters() if p.grad is not None}))
    (la, ga), (lb, gb), (lc, gc_) = grads
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(la, lc)
    assert set(ga) == set(gb) == set(gc_) and "to_cond_emb.weight" in ga
    for other in (gb, gc_):
        differ = [k for k in ga if k != "to_cond_emb.weight" and not torch.equal(ga[k], other[k])]
        assert not differ, differ
        # the table's gradient is summed with fp32 atomics: the tolerance tests/test_ops_gpu.py holds vbx_cond_emb_bwd to
        assert rel_err(other["to_cond_emb.weight"], ga["to_cond_emb.weight"].double().cpu()) < 1e-5
    assert float(ga["to_cond_emb.weight"].abs().max()) > 0
    # the lengths matter: the batch's one ratio (no token_lens) is another loss, and so is the step without lengths at all
    with rng_override(**draws):
        one_ratio = w_ids(lat, lens=FL, semantic_token_ids=ids).detach()
    assert not torch.equal(one_ratio, la)


def test_train_step_wave_lens_with_wav2vec_is_the_step_with_ids_and_token_lens():
    from voicebox_pytorch_amd.dp import TrainStep
    from voicebox_pytorch_amd.masks import rng_override

    w_tok, start, wave, ids, TL = _pair()
    w_tok.voicebox.load_state_dict(start)
    w_ids = _wrapper(state=start)
    lat, _, FL = w_ids.encode_raw_audio(wave, None, None, wave_lens=WAVE_LENS)
    draws, lr = _draws((3, 61, 100)), 1e-3
    # no clipping: the clip coefficient comes from the global gradient norm, which holds the table's gradient, summed with fp32
    # atomics -- its last bits differ from run to run and would reach every other parameter through g * coef
    ts1, ts2 = TrainStep(w_tok, lr=lr, max_grad_norm=None), TrainStep(w_ids, lr=lr, max_grad_norm=None)
    with rng_override(**draws):
        l1 = ts1.step(wave, wave_lens=WAVE_LENS)
    with rng_override(**draws):
        l2 = ts2.step(lat, lens=FL, cond_token_ids=ids, token_lens=TL)
    assert torch.isfinite(l1) and torch.equal(l1.detach(), l2.detach())
    sd1, sd2 = w_tok.voicebox.state_dict(), w_ids.voicebox.state_dict()
    differ = [k for k in sd1 if k != "to_cond_emb.weight" and not torch.equal(sd1[k], sd2[k])]
    assert not differ, differ
    assert not torch.equal(sd1["to_pred.weight"].cpu(), start["to_pred.weight"])

    # the table: the gradient this step scattered (the CEMB slice of the step's flat gradient buffer, which Adam read and left as
    # it was) between the two arms, with the tolerance tests/test_ops_gpu.py holds vbx_cond_emb_bwd to
    def table_grad(ts):
        lo = ts.fp.offsets["CEMB"]
        return ts.gflat[lo:lo + ts.fp.slots["CEMB"].numel()].view(ts.fp.slots["CEMB"].shape).detach().clone()

    g1, g2 = table_grad(ts1), table_grad(ts2)
    assert g1.shape == sd1["to_cond_emb.weight"].shape and float(g1.abs().max()) > 0
    assert rel_err(g2, g1.double().cpu()) < 1e-5, rel_err(g2, g1.double().cpu())
    # ... and it is the gradient of the lengths: the step with the batch's one ratio (no token_lens) scatters another
    w_one = _wrapper(state=start)
    ts3 = TrainStep(w_one, lr=lr, max_grad_norm=None)
    with rng_override(**draws):
        ts3.step(lat, lens=FL, cond_token_ids=ids)
    assert rel_err(table_grad(ts3), g1.double().cpu()) > 1e-3
    # a used row's first Adam step is lr * g / (|g| + eps): the rows the ids name moved, in both arms, and the same way wherever the
    # gradient is not within rounding of zero
    t1, t2, t0 = sd1["to_cond_emb.weight"], sd2["to_cond_emb.weight"], start["to_cond_emb.weight"].to(dev)
    assert not torch.equal(t1, t0) and not torch.equal(t2, t0)
    firm = g1.abs() > 1e-4 * g1.abs().max()
    assert firm.any() and torch.equal(torch.sign(t1 - t0)[firm], torch.sign(t2 - t0)[firm])
    assert torch.equal(torch.sign(t1 - t0)[firm], -torch.sign(g1)[firm])


def test_full_token_lens_is_the_call_without():
    """token_lens = T and lens = N on every row: the one ratio T / N of the plain entries, the same loss bit for bit"""
    from voicebox_pytorch_amd.masks import rng_override

    _, start, wave, ids, _ = _pair()
    w = _wrapper(state=start)
    lat = w.voicebox.audio_enc_dec.encode(wave)
    draws = _draws((3, 61, 100))
    with rng_override(**draws):
        a = w(lat, lens=[61] * 3, semantic_token_ids=ids).detach()
    with rng_override(**draws):
        b = w(lat, lens=[61] * 3, semantic_token_ids=ids, token_lens=[19] * 3).detach()
    assert torch.isfinite(a) and torch.equal(a, b)
