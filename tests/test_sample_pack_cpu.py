"""CPU (-m "not gpu"): sample(lens=, pack=True) -- the host plan of the packed row layout (voicebox_pytorch_amd/sample_pack.py,
include/vbx.h "packed rows") and every refusal of the public call, raised before any device call."""
import pytest
import torch

from voicebox_pytorch_amd import sample_pack as sp

LENGTH_SETS = [(1,), (111, 112, 113), (200, 47, 48, 49), (112, 113, 200, 49), (1, 111, 112, 113, 240, 5)]


@pytest.mark.parametrize("R", [0, 16])
@pytest.mark.parametrize("lens", LENGTH_SETS)
def test_pack_plan_properties(lens, R):
    N = max(lens) + 3
    plan = sp.pack_plan(lens, R, N=N)
    B = len(lens)
    sizes = [-(-(R + v) // 128) * 128 for v in lens]
    assert plan.Mp == sum(sizes) == sp.packed_rows(lens, R) and plan.Mp % 128 == 0
    assert plan.live_rows == sum(R + v for v in lens) and plan.dead_rows == plan.Mp - plan.live_rows and plan.padded_rows == B * (R + N)
    assert all(t.device.type == "cpu" for t in (plan.seg_start, plan.seg_klen, plan.tile_seg, plan.src_row, plan.dst_row))
    assert plan.seg_start.dtype == plan.seg_klen.dtype == plan.tile_seg.dtype == torch.int32
    # every seg_start is a multiple of 128, segments follow each other in batch order, seg_klen = R + len
    assert all(s % 128 == 0 for s in plan.seg_start.tolist())
    assert plan.seg_start.tolist() == [sum(sizes[:b]) for b in range(B)]
    assert plan.seg_klen.tolist() == [R + v for v in lens]
    # tile_seg agrees with the starts
    want_tiles = [b for b, s in enumerate(sizes) for _ in range(s // 128)]
    assert plan.tile_seg.tolist() == want_tiles
    # every live frame appears once in src_row; registers and dead rows are -1; dst_row is the inverse
    live = sorted(v for v in plan.src_row.tolist() if v >= 0)
    assert live == sorted(b * N + n for b, v in enumerate(lens) for n in range(v))
    assert (plan.src_row >= 0).sum() == sum(lens)
    for b, v in enumerate(lens):
        s0 = int(plan.seg_start[b])
        assert (plan.src_row[s0:s0 + R] == -1).all() and (plan.src_row[s0 + R + v:s0 + sizes[b]] == -1).all()
        assert plan.src_row[s0 + R:s0 + R + v].tolist() == [b * N + n for n in range(v)]
        assert plan.dst_row[b * N:b * N + v].tolist() == list(range(s0 + R, s0 + R + v)) and (plan.dst_row[b * N + v:(b + 1) * N] == -1).all()
        # the row's index inside its own [R + N] rotary table: registers 0 .. R-1, frame n at R + n, dead rows 0
        assert plan.local_row[s0:s0 + R + v].tolist() == list(range(R + v)) and not plan.local_row[s0 + R + v:s0 + sizes[b]].any()
    sp.check_tables(plan.seg_start, plan.seg_klen, plan.tile_seg, plan.Mp, B)
    # unpack(pack(x)) equals x on live frames and 0.0 elsewhere; register and dead rows of the packed tensor hold the fill
    gen = torch.Generator().manual_seed(len(lens) + R)
    x = torch.randn(B, N, 6, generator=gen)
    xp = sp.pack_rows(x, plan)
    assert xp.shape == (1, plan.Mp, 6) and not xp[0, plan.src_row < 0].any()
    back = sp.unpack_rows(xp, plan)
    keep = torch.arange(N)[None] < torch.tensor(lens)[:, None]
    assert back.shape == x.shape and torch.equal(back, x * keep[..., None])
    assert torch.equal(sp.unpack_rows(torch.full_like(xp, float("nan")), plan)[~keep], torch.zeros(int((~keep).sum()), 6))  # exactly 0.0
    m = torch.rand(B, N, generator=gen) < 0.5
    mp = sp.pack_rows(m, plan, fill=True)
    assert mp.dtype == torch.bool and mp[0, plan.src_row < 0].all() and torch.equal(sp.unpack_rows(mp, plan), m & keep)
    ids = torch.randint(1, 50, (B, N), generator=gen)
    assert torch.equal(sp.unpack_rows(sp.pack_rows(ids, plan), plan), ids * keep)


def test_bucket_arithmetic():
    R = 16
    assert sp.packed_rows((200, 47, 48, 49), R) == 256 + 128 + 128 + 128 == 640
    assert sp.packed_rows((112, 113, 200, 49), R) == 128 + 256 + 256 + 128 == 768
    assert sp.packed_rows((200, 47, 48, 49), R, 1024) == sp.packed_rows((130, 100, 47), R, 1024) == 1024
    assert sp.packed_rows((112,), R, 128) == 128 and sp.packed_rows((113,), R, 128) == 256 and sp.packed_rows((113,), R, 384) == 384
    plan = sp.pack_plan((130, 100, 47), R, 1024)
    assert plan.Mp == 1024 and plan.N == 130 and plan.tile_seg.tolist() == [0, 0, 1, 2, -1, -1, -1, -1]
    assert (plan.src_row[512:] == -1).all() and plan.dead_rows == 1024 - (146 + 116 + 63)
    sp.check_tables(plan.seg_start, plan.seg_klen, plan.tile_seg, 1024, 3)
    for bad in (0, -128, 64, 200, 128.0, True):
        with pytest.raises(ValueError, match="pack_bucket must be a positive multiple of 128"):
            sp.packed_rows((5,), R, bad)
    with pytest.raises(ValueError, match=">= 1"):
        sp.pack_plan((5, 0), R)


def test_check_tables_refuses_what_the_kernels_would_index_wrongly():
    plan = sp.pack_plan((200, 47), 16)
    ok = (plan.seg_start, plan.seg_klen, plan.tile_seg)

    def bad(i, idx, val):
        t = [x.clone() for x in ok]
        t[i][idx] = val
        return t

    for tables in (bad(0, 1, 200), bad(0, 1, 128), bad(1, 0, 0), bad(1, 1, 129), bad(2, 2, 2), bad(2, 2, -1), bad(2, 0, 1), bad(0, 1, 384)):
        with pytest.raises(ValueError, match="packed tables"):
            sp.check_tables(*tables, plan.Mp, 2)
    with pytest.raises(ValueError, match="packed tables"):
        sp.check_tables(*ok, plan.Mp + 64, 2)


def _cpu_wrapper(method="midpoint", **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=5, depth=2, dim_head=64, heads=2, condition_on_text=False, **kw)
    return vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=method)


def test_refusals_come_before_any_device_call():
    """every refusal of sample(pack=) on a CPU wrapper (no GPU, no engine): a message that names the way out"""
    from voicebox_pytorch_amd import engine

    cond = torch.randn(2, 8, 64)
    w = _cpu_wrapper()
    with pytest.raises(ValueError, match="pack=True needs lens"):
        w.sample(cond=cond, steps=3, pack=True)
    with pytest.raises(ValueError, match="pack_bucket only applies to pack=True"):
        w.sample(cond=cond, steps=3, lens=[8, 3], pack_bucket=128)
    for bad in (0, 64, 130, -128):
        with pytest.raises(ValueError, match="pack_bucket must be a positive multiple of 128"):
            w.sample(cond=cond, steps=3, lens=[8, 3], pack=True, pack_bucket=bad)
    with pytest.raises(ValueError, match="length_bucket pads frames that pack=True would drop"):
        w.sample(cond=cond, steps=3, lens=[8, 3], pack=True, length_bucket=64)
    with pytest.raises(NotImplementedError, match="dopri5 does not serve pack=True"):
        _cpu_wrapper("dopri5").sample(cond=cond, steps=3, lens=[8, 3], pack=True)
    with pytest.raises(NotImplementedError, match="GateLoop layers do not serve pack=True"):
        _cpu_wrapper(use_gateloop_layers=True).sample(cond=cond, steps=3, lens=[8, 3], pack=True)
    with engine.precise_mode():
        with pytest.raises(NotImplementedError, match="precise mode does not serve pack=True"):
            w.sample(cond=cond, steps=3, lens=[8, 3], pack=True)
    # lens are still validated first-hand, and a valid packed call on a CPU model meets the same refusal as any other: no fallback
    with pytest.raises(ValueError, match=r"lens\[1\] = 9"):
        w.sample(cond=cond, steps=3, lens=[8, 9], pack=True)
    from voicebox_pytorch_amd import _lib

    with pytest.raises((_lib.VbxError, RuntimeError, AssertionError)) as e:
        w.sample(cond=cond, steps=3, lens=[8, 3], pack=True, pack_bucket=256)
    assert not isinstance(e.value, (ValueError, NotImplementedError))
