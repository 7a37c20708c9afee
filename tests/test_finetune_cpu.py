"""CPU (-m "not gpu"): host logic of fine-tuning on the device -- frozen parameters in dp.TrainStep and LoRA adapters (lora.py).
 * the fp64 restatement tests/lora_ref.py against an independent autograd construction, and how far each planted fault moves it;
 * filtering and splitting of the fused Adam's segment table, the trainable range lists past 64 ranges, the adaLN mode rule;
 * every refusal, raised before anything is launched (there is no GPU here: a launch would fail loudly instead);
 * state dicts with adapters attached.
"""
import pytest
import torch

import lora_ref

SHAPES = [(64, 64, 1), (192, 64, 3), (340, 64, 8), (64, 170, 64)]  # (N, K, r) of the GPU kernel tests


def _rand(N, K, r, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g, dtype=torch.float64), torch.randn(r, K, generator=g, dtype=torch.float64) / K ** 0.5,
            torch.randn(N, r, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("N,K,r", SHAPES)
def test_restatement_equals_autograd(N, K, r):
    """W0 + s.B@A through F.linear in fp64, gradients by autograd: the restatement's merge, dA and dB to 1e-12."""
    w0, A, B, G = _rand(N, K, r, 1)
    alpha = 12.0
    A, B = A.requires_grad_(), B.requires_grad_()
    x = torch.randn(5, K, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    W = w0 + (alpha / r) * B @ A
    W.retain_grad()
    y = torch.nn.functional.linear(x, W)
    (y * torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))).sum().backward()
    Wr, _ = lora_ref.merge(w0, A.detach(), B.detach(), alpha)
    dA, dB, _, _ = lora_ref.grads(W.grad, A.detach(), B.detach(), alpha)
    assert float((Wr - W.detach()).abs().max()) <= 1e-12 * float(W.detach().abs().max())
    assert float((dA - A.grad).abs().max()) <= 1e-12 * float(A.grad.abs().max())
    assert float((dB - B.grad).abs().max()) <= 1e-12 * float(B.grad.abs().max())


def test_planted_faults_move_the_restatement():
    """alpha instead of alpha / r, A and B swapped, dA from W instead of dW, the scale missing in one gradient, the transposed product:
    each moves a result by >= 10 x the relative tolerance the GPU tests use (lora_ref.fault_tolerance: a tenth of the smallest
    movement, measured here and printed) -- and the kernels' own contract bounds, at the GPU tests' shapes, are far inside it."""
    moves = lora_ref.fault_movements()
    tol = lora_ref.fault_tolerance()
    for name, mv in moves.items():
        print(f"fault {name}: moves a result by {mv:.3e} (relative)")
    print(f"GPU tolerance (a tenth of the smallest movement): {tol:.3e}")
    assert set(moves) == set(lora_ref.FAULTS)
    assert all(mv >= 10 * tol for mv in moves.values()) and tol > 0
    for N, K, r in SHAPES:  # a kernel that meets its bound cannot hide a planted fault
        w0, A, B, G = _rand(N, K, r, 4)
        W, tw = lora_ref.merge(w0, A, B, 8.0)
        dA, dB, ta, tb = lora_ref.grads(G, A, B, 8.0)
        ba, bb = lora_ref.grad_bounds(ta, tb, N, K)
        assert float(lora_ref.merge_bound(tw, r).max() / W.abs().max()) < tol / 10
        assert float(ba.max() / dA.abs().max()) < tol / 10 and float(bb.max() / dB.abs().max()) < tol / 10


# ------------------------------------------------------------------------------------------- segment table
def _seg(off, count, cols=1, ld=0, dst=(0, 0, 0), rowmap=0, F=0):
    return dict(off=off, count=count, dst_bf16=dst[0], dst_f16=dst[1], dst_f32=dst[2], cols=cols, dst_ld=ld or cols, rowmap=rowmap, F=F, block0=0)


def test_adam_segment_table_filtering_and_splitting():
    from voicebox_pytorch_amd.dp import filter_adam_segments

    segs = [_seg(0, 4096, cols=64, dst=(1000, 2000, 0)),             # a packed matrix [64, 64]
            _seg(4096, 640),                                          # a plain run of small tensors
            _seg(4736, 4 * 128 * 32, cols=32, dst=(0, 50000, 0)),     # an adaLN weight block: four tensors of 128 rows
            _seg(21120, 512, cols=512, dst=(0, 0, 9000)),             # the one-row adaLN bias block: four tensors of 128
            _seg(21632, 2048, cols=64, ld=80, dst=(3000, 0, 0), rowmap=1, F=16)]
    same, blocks = filter_adam_segments(segs, [])
    assert [{k: v for k, v in s.items() if k != "block0"} for s in same] == [{k: v for k, v in s.items() if k != "block0"} for s in segs]
    assert blocks == 2 + 1 + 8 + 1 + 1 and [s["block0"] for s in same] == [0, 2, 3, 11, 12]
    frozen = [(0, 4096), (4096 + 128, 4096 + 192), (4736 + 128 * 32, 4736 + 2 * 128 * 32), (21120 + 384, 21120 + 512), (21632, 23680)]
    out, blocks = filter_adam_segments(segs, frozen)
    got = [(s["off"], s["count"], s["dst_bf16"], s["dst_f16"], s["dst_f32"], s["cols"]) for s in out]
    assert got == [(4096, 128, 0, 0, 0, 1), (4096 + 192, 640 - 192, 0, 0, 0, 1),
                   (4736, 128 * 32, 0, 50000, 0, 32), (4736 + 2 * 128 * 32, 2 * 128 * 32, 0, 50000 + 2 * 256 * 32, 0, 32),
                   (21120, 384, 0, 0, 9000, 384)]
    covered = torch.zeros(23680, dtype=torch.int32)
    for s in out:
        covered[s["off"]:s["off"] + s["count"]] += 1
    for lo, hi in frozen:
        assert int(covered[lo:hi].sum()) == 0  # nothing frozen is inside a segment
        covered[lo:hi] += 1
    assert bool((covered == 1).all())           # and everything else is, once
    assert [s["block0"] for s in out] == [0, 1, 2, 4, 8] and blocks == 9
    # factor-form adaLN blocks (rowmap 2) take no blocks of the launch, filtered or not
    segs[2]["rowmap"] = 2
    out, blocks = filter_adam_segments(segs, [(0, 4096)])
    assert blocks == 1 + 0 + 1 + 1
    with pytest.raises(AssertionError):
        filter_adam_segments(segs, [(21632 + 64, 21632 + 128)])  # a row-mapped matrix is one tensor: never split


def _tiny(depth=2, **kw):
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=64, depth=depth, heads=2, dim_head=64, condition_on_text=False, **kw)
    return vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb)


def test_trainable_ranges_and_chunks_past_64():
    from voicebox_pytorch_amd.dp import TrainStep, range_chunks, trainable_ranges

    vb, w = _tiny(depth=8)
    fp = vb.flat_params()
    names = list(fp.order)
    flags = [i % 2 == 0 for i in range(len(names))]  # every other slot: no two neighbours merge
    ranges = trainable_ranges(fp, flags)
    assert len(ranges) == sum(flags) > 64
    for (lo, hi), s in zip(ranges, [n for n, f in zip(names, flags) if f]):
        assert lo == fp.offsets[s] and hi == lo + (fp.slots[s].numel() + 3) // 4 * 4 and lo % 4 == 0 and hi <= fp.numel
    chunks = range_chunks(ranges)
    assert all(0 < len(c) <= 64 for c in chunks) and [r for c in chunks for r in c] == ranges and len(chunks) == -(-len(ranges) // 64)
    # all trainable: one range (neighbours merge across the slot padding); a block to exclude splits it
    assert trainable_ranges(fp, [True] * len(names)) == [(0, fp.numel)]
    lo = fp.offsets["L3.G1W"]
    hi = fp.offsets["L3.B2W"] + fp.slots["L3.B2W"].numel()
    assert trainable_ranges(fp, [True] * len(names), exclude=[(lo, hi)]) == [(0, lo), (hi, fp.numel)]
    # TrainStep re-derives the set when a flag flips (host comparison), and _wd_params follows
    ts = TrainStep(w, wd=0.1)
    assert ts._filter is None and len(ts._wd_params) == sum(p.ndim >= 2 for p in fp.slots.values())
    vb.to_pred.weight.requires_grad_(False)
    ts._refresh_trainable()
    assert ts._filter is not None and all(p is not vb.to_pred.weight for p in ts._wd_params)
    o = fp.offsets["PREDW"]
    assert all(not (lo <= o < hi) for lo, hi in ts._filter["ranges"]) and (o, o + 64 * 64) in ts._filter["frozen"]
    vb.to_pred.weight.requires_grad_(True)
    ts._refresh_trainable()
    assert ts._filter is None


def test_adaln_mode_rule():
    from voicebox_pytorch_amd.dp import TrainStep, adaln_rule

    vb, w = _tiny()
    fp = vb.flat_params()
    on = {s: True for s in fp.order}
    assert adaln_rule(on, 2) == "all"
    assert adaln_rule(dict(on, **{"L1.B2W": False}), 2) == "mixed"
    assert adaln_rule({s: not s.endswith(("G1W", "B1W", "G2W", "B2W")) for s in fp.order}, 2) == "none"
    ts = TrainStep(w, adaln_grads="factors")
    vb.transformer.layers[0][2].to_gamma.weight.requires_grad_(False)  # one adaLN weight frozen: mixed -> the gradient is materialised
    ts._refresh_trainable()
    assert ts._filter["adaln"] == "mixed" and ts.adaln_factors_apply(batch=2) is False
    for l in range(2):
        for i in (2, 4):
            vb.transformer.layers[l][i].to_gamma.weight.requires_grad_(False)
            vb.transformer.layers[l][i].to_beta.weight.requires_grad_(False)
    ts._refresh_trainable()
    assert ts._filter["adaln"] == "none"
    lo, hi = ts.adaln_weight_ranges()[0]
    assert all(b <= lo or a >= hi for a, b in ts._filter["ranges"])


# ------------------------------------------------------------------------------------------- refusals
def test_add_lora_refusals():
    import voicebox_pytorch_amd as vbx

    vb, w = _tiny()
    for bad in (0, 65, 2.5):
        with pytest.raises(NotImplementedError):
            vb.add_lora(rank=bad)
    with pytest.raises(ValueError):
        vb.add_lora(targets=("to_qkv", "to_embed"))
    with pytest.raises(NotImplementedError):
        vb.add_lora(targets=("to_qkva",))
    with pytest.raises(ValueError):
        vb.add_lora(layers=[2])
    with vbx.precise_mode():
        with pytest.raises(NotImplementedError):
            vb.add_lora()
    with pytest.raises(NotImplementedError):
        vbx.Transformer(dim=64, depth=2, heads=2).add_lora()
    assert vb._lora is None and not any("lora" in k for k in vb.state_dict())
    vb.add_lora(rank=4, alpha=8., layers=[1], targets=("to_out", "ff_in"))
    assert sorted(k for k in vb.state_dict() if "lora" in k) == [
        "transformer.layers.1.3.to_out.lora_A", "transformer.layers.1.3.to_out.lora_B", "transformer.layers.1.5.0.lora_A",
        "transformer.layers.1.5.0.lora_B"]
    assert vb.transformer.layers[1][5][0].lora_A.shape == (4, 64) and vb.transformer.layers[1][5][0].lora_B.shape == (340, 4)
    assert float(vb.transformer.layers[1][5][0].lora_B.abs().max()) == 0.0
    assert float(vb.transformer.layers[1][5][0].lora_A.abs().max()) <= 1.0 / 64 ** 0.5  # kaiming-uniform, a = sqrt(5): U(-1/sqrt(K), 1/sqrt(K))
    assert [n for n, p in vb.named_parameters() if p.requires_grad] == [
        "transformer.layers.1.3.to_out.lora_A", "transformer.layers.1.3.to_out.lora_B", "transformer.layers.1.5.0.lora_A",
        "transformer.layers.1.5.0.lora_B"]
    with pytest.raises(ValueError):
        vb.add_lora()  # a second one while attached
    # the eager autograd path names TrainStep, before anything is launched (no GPU here: a launch would raise VbxError instead)
    with pytest.raises(NotImplementedError, match="TrainStep"):
        w(torch.randn(2, 24, 64))


def test_train_step_refusals(monkeypatch):
    import torch.distributed as dist
    from voicebox_pytorch_amd.dp import TrainStep

    vb, w = _tiny()
    vb.to_pred.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="shard"):
        TrainStep(w, grad_mode="shard")
    vb.to_pred.weight.requires_grad_(True)
    ts = TrainStep(w, grad_mode="shard")  # nothing frozen: served as ever; a flag flipped later is refused at the next step
    vb.to_pred.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError):
        ts.step(torch.randn(2, 24, 64))
    vb.to_pred.weight.requires_grad_(True)
    vb.add_lora(rank=2)
    with pytest.raises(NotImplementedError, match="LoRA"):
        TrainStep(w, grad_mode="shard")
    monkeypatch.setenv("VBX_FORCE_DIST", "1")
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.HashStore())
    try:
        with pytest.raises(NotImplementedError, match="exchange"):
            TrainStep(w, broadcast_params=False)
        vb.detach_lora()
        TrainStep(w, broadcast_params=False)  # plain model: the forced exchange is served as ever
    finally:
        dist.destroy_process_group()


def test_lora_plan_checks_every_range():
    from voicebox_pytorch_amd import _lib
    from voicebox_pytorch_amd.lora import LoraTable

    ok = LoraTable([(0, 0, 0, 256, 64, 64, 3, 0.5), (4096, 4096, 512, 1024, 340, 64, 3, 0.5)], 4096 + 340 * 64, 4096 + 340 * 64, 1024 + 340 * 3)
    assert ok.apply_blocks == 2 + 11 and ok.grad_tiles == 1 + 3 and ok.max_rank == 3 and ok.max_k == 64
    assert ok.scratch_floats == (1 * 3 * 64 + 1 * 64 * 3) + (3 * 3 * 64 + 1 * 340 * 3)
    for bad in ([(0, 0, 0, 256, 64, 64, 3, 0.5)], 4095, 4096, 1024), ([(0, 0, 0, 256, 64, 64, 3, 0.5)], 4096, 4095, 1024), \
               ([(0, 0, 0, 256, 64, 64, 3, 0.5)], 4096, 4096, 256 + 64 * 3 - 1), ([(0, 0, 0, 256, 64, 64, 65, 0.5)], 4096, 4096, 1 << 20), \
               ([(-4, 0, 0, 256, 64, 64, 3, 0.5)], 4096, 4096, 1024):
        with pytest.raises(_lib.VbxError):
            LoraTable(*bad)


# ------------------------------------------------------------------------------------------- state dicts
def test_state_dicts_with_adapters_attached():
    from voicebox_pytorch_amd import _lib

    vb, w = _tiny()
    sd0 = {k: v.clone() for k, v in vb.state_dict().items()}
    flags0 = {n: p.requires_grad for n, p in vb.named_parameters()}
    vb.add_lora(rank=3, alpha=6.)
    sd = vb.state_dict()
    assert set(sd) - set(sd0) == {k for k in sd if k.endswith((".lora_A", ".lora_B"))} and len(set(sd) - set(sd0)) == 16
    assert all(torch.equal(sd[k], sd0[k]) for k in sd0)  # W0 under the reference's keys
    assert set(vb.lora_state_dict()) == set(sd) - set(sd0)
    assert all(k.startswith("voicebox.") or "lora" not in k for k in w.state_dict())
    # a plain dict loads as the new base (strict), the adapters stay
    new = {k: v + 1.0 for k, v in sd0.items()}
    vb.load_state_dict(new)
    assert all(torch.equal(vb.state_dict()[k], new[k]) for k in new)
    assert torch.equal(vb.state_dict()["transformer.layers.0.3.to_qkv.lora_A"], sd["transformer.layers.0.3.to_qkv.lora_A"])
    # B = 0 so far: nothing is pending beyond a merge that changes no bit; a loaded non-zero B on a CPU model cannot be merged here
    lsd = {k: torch.ones_like(v) for k, v in vb.lora_state_dict().items()}
    vb.load_lora_state_dict(lsd)
    assert vb._lora.needs_apply
    with pytest.raises(_lib.VbxError):
        vb.merge_lora()
    with pytest.raises(ValueError):
        vb.load_lora_state_dict({k: v for k, v in list(lsd.items())[1:]})
    vb.detach_lora()  # W0 back, bit for bit; a plain model with the flags of before
    assert set(vb.state_dict()) == set(sd0) and all(torch.equal(vb.state_dict()[k], new[k]) for k in new)
    assert {n: p.requires_grad for n, p in vb.named_parameters()} == flags0
    with pytest.raises(ValueError):
        vb.detach_lora()
