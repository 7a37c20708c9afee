"""GPU: the EMA of the weights that dp.TrainStep(ema_decay=) keeps inside its Adam launches.

Kernel level -- vbx_adam_step_packed_ema, vbx_adam_adaln_factors_ema and vbx_adam_step_ema on the cases of tests/optim_check.py, each at
the decays 0, 0.9 and 0.9999: p, m, v and every operand copy bit-equal to the entry point without _ema from the same inputs,
optim_check's own checks still passing, and the average against tests/ema_check.py teacher-forced on the device's p' (bound, the exact
rules, untouched elements and guards keeping their bits); vbx_swap_f32; the host refusals.
Model level (dim 64 / depth 2 / heads 2, 2 x 24 frames, 4 steps, ema_update_after_step=1, ema_decay=0.9) -- training is unchanged bit
for bit, the average passes check_ema after every step over the whole buffer on every launch path, ema_weights() serves the average to
state_dict() and sample() and restores the weights, frozen tensors, LoRA adapters, the trainer's checkpoint, the refusals."""
import ctypes as C
import multiprocessing as mp
import os
import socket
import sys

import pytest
import torch

import ema_check as ec
import optim_check as oc
from ema_check import DECAYS, PLAIN_NS, SWAP_CASES
from optim_check import FACTOR_CASES, PACKED_CASES, TABLES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = "cuda"
HYPER = (oc.LR, oc.B1, oc.B2, oc.EPS)
B_, N_, D_ = 2, 24, 64
STEPS, AFTER, DECAY = 4, 1, 0.9


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib, engine

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    engine._rt()  # the prototypes of the stage-level entry points
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def cpu(d):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in d.items()}


def _gs(gs):
    return None if gs is None else torch.tensor([gs], device=dev)


def _ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def _longs(xs):
    return (C.c_long * len(xs))(*xs)


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(oc.bits(a[k]), oc.bits(b[k])), f"{what}: {k} differs from the entry point without _ema"


# ----------------------------------------------------------------------------- A. vbx_adam_step_packed_ema
def _device_table(table, dst):
    from voicebox_pytorch_amd.engine import VbxAdamSeg

    tab = (VbxAdamSeg * len(table.segs))()
    for row, s in zip(tab, table.segs):
        for f in oc.SEG_FIELDS:
            if f in ("dst_bf16", "dst_f16", "dst_f32"):
                setattr(row, f, _ptr(dst[table.resolve(s[f])[0]], table.resolve(s[f])[1]) if s[f] else None)
            else:
                setattr(row, f, s[f])
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)


def _packed_run(L, case, ema=None, d=0.0):
    table, inp = TABLES[case.table], oc.packed_inputs(case)
    state = {k: inp[k].to(dev) for k in "pmv"}
    dst = {n: t.to(dev) for n, t in oc.new_dst(table).items()}
    raw, g, gs = _device_table(table, dst), inp["g"].to(dev), _gs(case.gs)
    tail = (raw.data_ptr(), len(table.segs), table.total_blocks, *HYPER, case.step, gs.data_ptr() if gs is not None else None, st())
    head = (state["p"].data_ptr(), g.data_ptr(), state["m"].data_ptr(), state["v"].data_ptr())
    rc = L.lib().vbx_adam_step_packed(*head, *tail) if ema is None else L.lib().vbx_adam_step_packed_ema(*head, ema.data_ptr(), d, *tail)
    assert rc == 0, L.lib().vbx_last_error().decode()
    return cpu({**state, **dst})


@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: c.name)
def test_adam_step_packed_ema(L, case):
    table = TABLES[case.table]
    old = _packed_run(L, case)
    e_old = ec.packed_ema(case)
    for d in DECAYS:
        ema = e_old.to(dev)
        got = _packed_run(L, case, ema, d)
        _same_bits(old, got, f"{case.name} d={d}")
        oc.check_packed(case, got)
        e_new = ema.cpu()
        ec.check_ema(f"{case.name}-d{d}", got["p"], e_old, e_new, d, table.covered())
        again = e_old.to(dev)
        _packed_run(L, case, again, d)
        assert torch.equal(oc.bits(again.cpu()), oc.bits(e_new)), "a rerun differs"


# ----------------------------------------------------------------------------- B. vbx_adam_adaln_factors_ema
def _factor_run(L, case, ema=None, d=0.0):
    lay, inp = oc.factor_inputs(case)
    state = {k: inp[k].to(dev) for k in "pmv"}
    fdst = {n: t.to(dev) for n, t in oc.new_factor_dst(lay).items()}
    (db, do), (tb, to) = oc.embed_nan(inp["dada"]), oc.embed_nan(inp["temb"])
    db, tb, gs = db.to(dev), tb.to(dev), _gs(case.gs)
    ptrs = (C.c_void_p * lay["L"])(*[(_ptr(fdst[f"f16.{l}"]) if f"f16.{l}" in fdst else None) for l in range(lay["L"])])
    head = (state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr())
    tail = (_longs(lay["w_off"]), ptrs if lay["dst_array"] else None, _ptr(db, do), _ptr(tb, to), lay["L"], case.B, lay["J4"], lay["Th"],
            *HYPER, case.step, gs.data_ptr() if gs is not None else None, st())
    rc = L.lib().vbx_adam_adaln_factors(*head, *tail) if ema is None else L.lib().vbx_adam_adaln_factors_ema(*head, ema.data_ptr(), d, *tail)
    assert rc == 0, L.lib().vbx_last_error().decode()
    return cpu({**state, **fdst})


@pytest.mark.parametrize("case", FACTOR_CASES, ids=lambda c: c.name)
def test_adam_adaln_factors_ema(L, case):
    lay, _ = oc.factor_inputs(case)
    old = _factor_run(L, case)
    e_old = ec.factor_ema(case)
    for d in DECAYS:
        ema = e_old.to(dev)
        got = _factor_run(L, case, ema, d)
        _same_bits(old, got, f"{case.name} d={d}")
        oc.check_factor(case, got)
        e_new = ema.cpu()
        ec.check_ema(f"{case.name}-d{d}", got["p"], e_old, e_new, d, oc.factor_covered(lay))
        again = e_old.to(dev)
        _factor_run(L, case, again, d)
        assert torch.equal(oc.bits(again.cpu()), oc.bits(e_new)), "a rerun differs"


# ----------------------------------------------------------------------------- C. vbx_adam_step_ema
def _plain_run(L, n, ema=None, d=0.0, step=2):
    inp, _ = ec.plain_inputs(n)
    state = {k: inp[k].to(dev) for k in "pmv"}
    g, gs = inp["g"].to(dev), _gs(oc.GSCALES[1])
    if ema is None:
        L.call("vbx_adam_step", state["p"], g, state["m"], state["v"], n, *HYPER, step, gs, st())
    else:
        L.call("vbx_adam_step_ema", state["p"], g, state["m"], state["v"], ema, d, n, *HYPER, step, gs, st())
    return cpu(state)


@pytest.mark.parametrize("n", PLAIN_NS)
def test_adam_step_ema(L, n):
    inp, cov = ec.plain_inputs(n)
    old = _plain_run(L, n)
    for d in DECAYS:
        ema = inp["e"].to(dev)
        got = _plain_run(L, n, ema, d)
        _same_bits(old, got, f"plain n={n} d={d}")
        e_new = ema.cpu()
        ck = ec.check_ema(f"plain-n{n}-d{d}", got["p"], inp["e"], e_new, d, cov, done=False)
        oc.check_untouched(ck, inp, got, cov)
        ck.done()
        again = inp["e"].to(dev)
        _plain_run(L, n, again, d)
        assert torch.equal(oc.bits(again.cpu()), oc.bits(e_new)), "a rerun differs"


# ----------------------------------------------------------------------------- D. vbx_swap_f32
@pytest.mark.parametrize("n,oa,ob", SWAP_CASES)
def test_swap_f32(L, n, oa, ob):
    a0, b0 = ec.swap_inputs(n, oa, ob)
    a, b = a0.to(dev), b0.to(dev)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    rc = L.lib().vbx_swap_f32(_ptr(a, oa), _ptr(b, ob), n, st())
    assert rc == 0, L.lib().vbx_last_error().decode()
    a1, b1 = a.cpu(), b.cpu()
    want_a, want_b = a0.clone(), b0.clone()
    want_a[oa: oa + n], want_b[ob: ob + n] = b0[ob: ob + n], a0[oa: oa + n]
    assert torch.equal(oc.bits(a1), oc.bits(want_a)) and torch.equal(oc.bits(b1), oc.bits(want_b))  # exact, guards intact


# ----------------------------------------------------------------------------- E. host refusals
def test_host_refusals_launch_nothing(L):
    """ema = NULL, an ema that is not aligned like p, a decay outside [0, 1) and n <= 0 are answered with an error code; nothing is written."""
    lib = L.lib()
    case = PACKED_CASES[0]
    table, inp = TABLES[case.table], oc.packed_inputs(case)
    state = {k: inp[k].to(dev) for k in "pmv"}
    dst = {n: t.to(dev) for n, t in oc.new_dst(table).items()}
    raw, g = _device_table(table, dst), inp["g"].to(dev)
    ema = torch.cat((ec.packed_ema(case), torch.zeros(4))).to(dev)

    def packed(e, d=0.9, blocks=table.total_blocks):
        return lib.vbx_adam_step_packed_ema(state["p"].data_ptr(), g.data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), e, d,
                                            raw.data_ptr(), len(table.segs), blocks, *HYPER, 1, None, st())

    assert packed(None) != 0 and packed(_ptr(ema, 1)) != 0 and packed(ema.data_ptr(), 1.0) != 0 and packed(ema.data_ptr(), -0.5) != 0
    assert packed(ema.data_ptr(), 0.9, 0) != 0 and packed(state["p"].data_ptr()) != 0

    def plain(e, n=64, d=0.9):
        return lib.vbx_adam_step_ema(state["p"].data_ptr(), g.data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), e, d, n, *HYPER, 1,
                                     None, st())

    assert plain(None) != 0 and plain(_ptr(ema, 1)) != 0 and plain(ema.data_ptr(), 0) != 0 and plain(ema.data_ptr(), -4) != 0
    assert plain(ema.data_ptr(), 64, 1.5) != 0
    lay = oc.factor_layout(2, 8, 8)
    none = (C.c_void_p * 2)(None, None)
    dada, temb = torch.ones(2 * 3 * 8 + 8, device=dev), torch.ones(3 * 8 + 8, device=dev)

    def factor(e, d=0.9):
        return lib.vbx_adam_adaln_factors_ema(state["p"].data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), e, d, _longs(lay["w_off"]),
                                              none, dada.data_ptr(), temb.data_ptr(), 2, 3, 8, 8, *HYPER, 1, None, st())

    assert factor(None) != 0 and factor(_ptr(ema, 2)) != 0 and factor(ema.data_ptr(), 1.0) != 0
    assert lib.vbx_swap_f32(ema.data_ptr(), state["p"].data_ptr(), 0, st()) != 0
    assert lib.vbx_swap_f32(ema.data_ptr(), None, 8, st()) != 0
    assert lib.vbx_swap_f32(ema.data_ptr(), _ptr(ema, 4), 8, st()) != 0  # overlapping
    got = cpu({**state, **dst, "ema": ema[:-4]})
    for k in "pmv":
        assert torch.equal(oc.bits(got[k]), oc.bits(inp[k]))
    assert torch.equal(oc.bits(got["ema"]), oc.bits(ec.packed_ema(case)))
    for n, t in oc.new_dst(table).items():
        assert torch.equal(oc.bits(got[n]), oc.bits(t))
    assert packed(ema.data_ptr()) == 0  # (the same call within the contract is served)
    torch.cuda.synchronize()


# ============================================================================= model level
def _model(seed=0):
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(seed)
    vb = vbx.VoiceBox(dim=D_, depth=2, heads=2, dim_head=64, condition_on_text=False)
    g = torch.Generator().manual_seed(seed + 100)  # the reference zero-initialises the adaLN projections: move them
    with torch.no_grad():
        for n, p in vb.named_parameters():
            if ".to_gamma." in n or ".to_beta." in n:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    vb = vb.to(dev)
    return vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def _draws(seed):
    g = torch.Generator().manual_seed(seed)
    return dict(x1=torch.randn(B_, N_, D_, generator=g), x0=torch.randn(B_, N_, D_, generator=g), times=torch.rand(B_, generator=g),
                frac_lengths=0.7 + 0.3 * torch.rand(B_, generator=g), rand=torch.rand(B_, generator=g))


def _call(ts, d, how="step", *args, **kw):
    from voicebox_pytorch_amd.masks import rng_override

    with rng_override(**{k: v for k, v in d.items() if k != "x1"}):
        return getattr(ts, how)(d["x1"].to(dev), *args, **kw)


def _advance(ts, i, mode):
    """optimizer step i (0-based) in the given mode; returns the loss of its last micro-batch"""
    if mode == "accumulate":
        _call(ts, _draws(300 + i), "accumulate", 0.5)
        return _call(ts, _draws(20 + i), "accumulate_last_and_apply", 0.5)
    return _call(ts, _draws(20 + i))


def _pair(seed, ema_kw=None, prepare=None, **kw):
    """(vb, wrapper, TrainStep with EMA), (the twin without) from the same seeds"""
    from voicebox_pytorch_amd.dp import TrainStep

    out = []
    for with_ema in (True, False):
        vb, w = _model(seed)
        if prepare is not None:
            prepare(vb)
        extra = dict(ema_decay=DECAY, ema_update_after_step=AFTER, **(ema_kw or {})) if with_ema else {}
        out.append((vb, w, TrainStep(w, lr=1e-3, **kw, **extra)))
    return out


def _check_step(ts, t, e_prev, name, touched=None):
    """step.ema after optimizer step t against the snapshot of before it and this step's flat, over the whole buffer"""
    torch.cuda.synchronize()
    d = ec.f32(ts.ema_decay_at(t))
    flat, ema = ts.fp.flat.detach().cpu(), ts.ema.detach().cpu()
    ec.check_ema(f"{name}-step{t}", flat, e_prev, ema, d, touched)
    if t <= AFTER:
        assert d == 0.0 and torch.equal(oc.bits(ema), oc.bits(flat)), "the first step leaves a copy of the weights"
    return ema


@pytest.mark.parametrize("mode", ["auto", "materialize", "fused0", "accumulate"])
def test_training_is_unchanged_and_the_average_follows(mode, monkeypatch):
    """Loss and flat after every step bit-equal to a twin TrainStep without EMA; step.ema passes check_ema over the whole buffer (the
    real segment table; with "auto" the factor launch in situ); step 1 (t <= ema_update_after_step) leaves ema bit-equal to flat."""
    if mode == "fused0":
        monkeypatch.setenv("VBX_FUSED_ADAM", "0")
    kw = dict(adaln_grads="materialize") if mode == "materialize" else {}
    (vb, w, ts), (vb2, w2, ts2) = _pair(1, **kw)
    assert ts2.ema is None and torch.equal(oc.bits(ts.ema.cpu()), oc.bits(ts.fp.flat.detach().cpu()))
    assert ts.adaln_factors_apply(batch=B_) == (mode != "materialize")  # "auto": the factor-form launch runs in situ
    e_prev = ts.ema.detach().cpu().clone()
    for i in range(STEPS):
        la, lb = _advance(ts, i, mode), _advance(ts2, i, mode)
        assert float(la) == float(lb), f"step {i + 1}: the loss differs from the twin without EMA"
        assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(ts2.fp.flat.detach().cpu())), f"step {i + 1}: flat differs"
        e_prev = _check_step(ts, i + 1, e_prev, f"model-{mode}")
    assert ts.steps == STEPS and not torch.equal(ts.ema.cpu(), ts.fp.flat.detach().cpu())
    assert torch.equal(oc.bits(ts.m.cpu()), oc.bits(ts2.m.cpu())) and torch.equal(oc.bits(ts.v.cpu()), oc.bits(ts2.v.cpu()))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _forced_exchange_worker(port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["VBX_FORCE_DIST"] = "1"
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))  # nccl == RCCL on ROCm
    (vb, w, ts), (vb2, w2, ts2) = _pair(2, bucket_bytes=1 << 16)
    assert ts.exchange and ts.comm_stream is not None and ts2.exchange
    e_prev = ts.ema.detach().cpu().clone()
    for i in range(STEPS):
        la, lb = _advance(ts, i, "auto"), _advance(ts2, i, "auto")
        assert float(la) == float(lb)
        assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(ts2.fp.flat.detach().cpu()))
        e_prev = _check_step(ts, i + 1, e_prev, "model-forced-exchange")
    torch.cuda.synchronize()
    dist.destroy_process_group()
    torch.save(dict(steps=ts.steps, exchange=bool(ts.exchange)), out)


def test_average_under_the_forced_exchange_path(tmp_path):
    """VBX_FORCE_DIST=1 at world size 1 (as tests/test_dp_gpu.py::test_rccl_path_executes_at_world_size_1 sets it up): the all-reduce
    path's Adam launch takes the _ema entry point too -- one update per optimizer step, training unchanged."""
    out = str(tmp_path / "forced.pt")
    p = mp.get_context("spawn").Process(target=_forced_exchange_worker, args=(_free_port(), out))
    p.start()
    p.join(300)
    assert p.exitcode == 0, p.exitcode
    res = torch.load(out)
    assert res["exchange"] and res["steps"] == STEPS


def _sample(w, cond):
    torch.manual_seed(7)
    return w.sample(cond=cond, steps=4).clone()


def _sd_equal(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(oc.bits(a[k].detach().cpu()), oc.bits(b[k].detach().cpu())), k


def test_ema_weights_serves_the_average_and_restores_the_weights():
    (vb, w, ts), (vb2, w2, ts2) = _pair(3)
    cond = torch.randn(B_, N_, D_, generator=torch.Generator().manual_seed(11)).to(dev)
    for i in range(STEPS - 1):
        assert float(_advance(ts, i, "auto")) == float(_advance(ts2, i, "auto"))
    outside = _sample(w, cond)  # a sampler and its graph exist before the context is entered
    assert torch.equal(outside, _sample(w, cond))
    before = ts.fp.flat.detach().clone()
    ema_sd = ts.ema_state_dict()
    live_sd = {k: v.detach().clone() for k, v in vb.state_dict().items()}
    with ts.ema_weights():
        _sd_equal(vb.state_dict(), ema_sd)
        _sd_equal(ts.ema_state_dict(), ema_sd)
        inside = _sample(w, cond)
        with pytest.raises(RuntimeError):
            with ts.ema_weights():
                pass
        for how, args in (("step", ()), ("accumulate", (0.5,)), ("accumulate_last_and_apply", (0.5,))):
            with pytest.raises(RuntimeError):
                _call(ts, _draws(50), how, *args)
        with pytest.raises(RuntimeError):
            ts.apply_accumulated()
    assert not torch.equal(inside, outside)
    vb3, w3 = _model(99)
    vb3.load_state_dict(ema_sd)
    assert torch.equal(oc.bits(inside.cpu()), oc.bits(_sample(w3, cond).cpu())), "the sample inside differs from a fresh model's"
    assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(before.cpu())), "flat after exit"
    _sd_equal(vb.state_dict(), live_sd)
    assert torch.equal(oc.bits(_sample(w, cond).cpu()), oc.bits(outside.cpu()))
    with pytest.raises(KeyError):  # exit after an exception restores as well
        with ts.ema_weights():
            raise KeyError("inside")
    assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(before.cpu())) and not ts._ema_swapped
    assert float(_advance(ts, STEPS - 1, "auto")) == float(_advance(ts2, STEPS - 1, "auto")), "the step after the context"
    assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(ts2.fp.flat.detach().cpu()))
    # load_ema_state_dict: the inverse; a shape mismatch is refused before anything is copied
    kept = ts.ema.detach().clone()
    sd = ts.ema_state_dict()
    ts.ema.zero_()
    bad = dict(sd)
    last = [k for k in ts._ema_views() if sd[k].ndim == 2][-1]
    bad[last] = bad[last][:, :-1]
    with pytest.raises(ValueError):
        ts.load_ema_state_dict(bad)
    assert float(ts.ema.abs().max()) == 0.0
    ts.load_ema_state_dict(sd)
    used = torch.zeros(ts.fp.numel, dtype=torch.bool)
    for s in ts.fp.order:
        used[ts.fp.offsets[s]: ts.fp.offsets[s] + ts.fp.slots[s].numel()] = True
    assert torch.equal(oc.bits(ts.ema.cpu())[used], oc.bits(kept.cpu())[used])
    ts.ema_reset()
    assert torch.equal(oc.bits(ts.ema.cpu()), oc.bits(ts.fp.flat.detach().cpu()))


def test_frozen_tensors_average_stands_still():
    """transformer.layers[0] frozen: that range of step.ema keeps its bits over all steps (it is not touched), the rest passes check_ema."""
    def freeze(vb):
        for p in vb.transformer.layers[0].parameters():
            p.requires_grad_(False)

    (vb, w, ts), (vb2, w2, ts2) = _pair(4, prepare=freeze)
    fp = ts.fp
    frozen = torch.zeros(fp.numel, dtype=torch.bool)
    for s in fp.order:
        if not fp.slots[s].requires_grad:
            frozen[fp.offsets[s]: fp.offsets[s] + fp.slots[s].numel()] = True
    assert bool(frozen.any()) and not bool(frozen.all())
    start = ts.ema.detach().cpu().clone()
    e_prev = start.clone()
    for i in range(STEPS):
        assert float(_advance(ts, i, "auto")) == float(_advance(ts2, i, "auto"))
        # (the padding between slots is untouched as well; check_ema's bit rule for untouched elements holds for it either way)
        e_prev = _check_step(ts, i + 1, e_prev, "model-frozen", touched=~frozen)
        assert torch.equal(oc.bits(e_prev)[frozen], oc.bits(start)[frozen])
    assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(ts2.fp.flat.detach().cpu()))


def test_lora_adapters_are_averaged():
    (vb, w, ts), (vb2, w2, ts2) = _pair(5, prepare=lambda vb: vb.add_lora(rank=4))
    lo = ts._lora_rt
    lflat = lo["state"].ensure(ts.fp.flat.device)
    assert torch.equal(oc.bits(lo["ema"].cpu()), oc.bits(lflat.detach().cpu()))
    e_prev = lo["ema"].detach().cpu().clone()
    base0 = ts.ema.detach().cpu().clone()
    for i in range(STEPS):
        assert float(_advance(ts, i, "auto")) == float(_advance(ts2, i, "auto"))
        torch.cuda.synchronize()
        assert ts._lora_rt is lo
        d = ec.f32(ts.ema_decay_at(i + 1))
        e_new = lo["ema"].detach().cpu().clone()
        ec.check_ema(f"model-lora-step{i + 1}", lflat.detach().cpu(), e_prev, e_new, d)
        e_prev = e_new
    assert not torch.equal(e_prev, lflat.detach().cpu())
    assert torch.equal(oc.bits(ts.ema.cpu()), oc.bits(base0))  # the base is frozen: its average is not touched
    assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(ts2.fp.flat.detach().cpu()))
    before = ts.fp.flat.detach().clone()
    ema_sd = ts.ema_state_dict()
    assert any(k.endswith("lora_A") for k in ema_sd)
    vb3, w3 = _model(77)
    vb3.add_lora(rank=4)
    vb3.load_state_dict(ema_sd)
    flat3 = vb3.flat_params().flat
    with ts.ema_weights():
        _sd_equal(vb.state_dict(), ema_sd)
        for e in lo["state"].entries:
            o, n = ts.fp.offsets[e["slot"]], e["N"] * e["K"]
            assert torch.equal(oc.bits(ts.fp.flat[o:o + n].detach().cpu()), oc.bits(flat3[o:o + n].detach().cpu())), (e["slot"], "W_eff of the average")
        assert not torch.equal(ts.fp.flat.detach(), before)
    assert torch.equal(oc.bits(ts.fp.flat.detach().cpu()), oc.bits(before.cpu())), "W_eff after exit"
    assert float(_advance(ts, STEPS, "auto")) == float(_advance(ts2, STEPS, "auto"))


class _Latents(torch.utils.data.Dataset):
    def __init__(self, n=8):
        g = torch.Generator().manual_seed(5)
        self.x = [torch.randn(N_, D_, generator=g) for _ in range(n)]

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i]


def _nested_equal(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _nested_equal(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _nested_equal(x, y, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), path
    else:
        assert a == b, path


def test_trainer_checkpoint_and_validation(tmp_path):
    import voicebox_pytorch_amd as vbx

    hyper = dict(ema_decay=DECAY, ema_update_after_step=AFTER, ema_inv_gamma=1.0, ema_power=None)

    def trainer(seed, folder, **kw):
        vb, w = _model(seed)
        torch.manual_seed(0)
        return vbx.VoiceBoxTrainer(w, batch_size=2, dataset=_Latents(), num_train_steps=10, lr=1e-3, valid_frac=0.25, log_every=1000,
                                   save_results_every=1, save_model_every=1000, results_folder=str(folder), length_bucket=0, **kw)

    tr, tw = trainer(6, tmp_path / "a", **hyper), trainer(6, tmp_path / "b")
    for t in (tr, tw):
        torch.manual_seed(1)
        for i in range(3):
            logs = t.train_step()
            assert ("valid_loss_ema" in logs) == (t is tr) and "valid_loss" in logs
            if t is tr:  # the same batch and draws; optimizer step 1 <= ema_update_after_step left the average equal to the weights
                assert (logs["valid_loss_ema"] == logs["valid_loss"]) == (i == 0), (i, logs)
    pa, pb = str(tmp_path / "voicebox.3.pt"), str(tmp_path / "twin.3.pt")
    tr.save(pa)
    tw.save(pb)
    A, Bp = torch.load(pa, map_location="cpu"), torch.load(pb, map_location="cpu")
    assert set(A) == {"model", "optim", "scheduler", "ema_model", "ema"} and set(Bp) == {"model", "optim", "scheduler"}
    for k in ("model", "optim", "scheduler"):
        _nested_equal(A[k], Bp[k], k)
    assert A["ema"] == hyper
    ts = tr.train_step_fn
    _sd_equal(A["ema_model"], ts.ema_state_dict())
    assert any(not torch.equal(A["ema_model"][k], A["model"]["voicebox." + k]) for k in A["ema_model"] if "voicebox." + k in A["model"])
    # the average round-trips bit for bit
    t3 = trainer(7, tmp_path / "c", **hyper)
    t3.load(pa)
    _sd_equal(t3.train_step_fn.ema_state_dict(), A["ema_model"])
    assert t3.train_step_fn.steps == 3
    # a file without the EMA keys loads and leaves ema == flat
    t4 = trainer(8, tmp_path / "d", **hyper)
    t4.load(pb)
    assert torch.equal(oc.bits(t4.train_step_fn.ema.cpu()), oc.bits(t4.train_step_fn.fp.flat.detach().cpu()))
    # a file written with EMA loads into a trainer without it
    t5 = trainer(9, tmp_path / "e")
    t5.load(pa)
    assert t5.train_step_fn.ema is None
    assert torch.equal(oc.bits(t5.train_step_fn.fp.flat.detach().cpu()), oc.bits(tr.train_step_fn.fp.flat.detach().cpu()))


def test_refusals():
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _model(0)
    with pytest.raises(NotImplementedError):
        TrainStep(w, grad_mode="shard", ema_decay=0.9)
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=0.9, ema_power=0.0), dict(ema_decay=0.9, ema_power=-2.0)):
        with pytest.raises(ValueError):
            TrainStep(w, **bad)
    plain = TrainStep(w)
    assert plain.ema is None and plain.ema_hyper is None
    for call in (plain.ema_weights, plain.ema_state_dict, plain.ema_reset):
        with pytest.raises(RuntimeError):
            call()
