"""The per-tile error metric of the attention tests (tests/attn_check.py) on CPU: errors confined to one tail tile pass the global
bounds of tests/test_ops_gpu.py::test_attn_fwd_bwd and are rejected per tile; tiles whose reference is exactly zero must be exactly
zero."""
import math

import torch

from attn_check import BOUNDS, Checks, attn_inputs, rel_err, tile_errors, worst_tile
from oracle import restate


def _confine(ref, b, h, rows, frac, seed):
    """ref with an error of relative size `frac` added to rows `rows` of (b, h) only."""
    got = ref.clone()
    tile = ref[b, h, rows]
    u = torch.randn(tile.shape, generator=torch.Generator().manual_seed(seed), dtype=ref.dtype)
    got[b, h, rows] = tile + frac * tile.norm() * u / u.norm()
    return got


def test_forward_tail_error_hides_under_the_global_bound():
    """2 % on one head's 5-row tail tile at (B, H, Np) = (1, 2, 1029), the reference's temperature."""
    q, k, v = (t.double() for t in attn_inputs(1, 2, 1029, seed=1031))
    ref = restate.attend(q, k, v, scale=10.0)
    got = _confine(ref, 0, 1, slice(1024, 1029), 0.02, seed=1)
    assert rel_err(got, ref) < 1.5e-3, rel_err(got, ref)  # test_attn_fwd_bwd's out16 bound: accepted
    err, idx = worst_tile(tile_errors(got, ref))
    assert idx == (0, 1, 8) and abs(err - 0.02) < 1e-9, (err, idx)
    assert err > BOUNDS["qknorm"]["out16_tile"] and err > BOUNDS["spread"]["out16_tile"]  # rejected per tile
    assert float(tile_errors(got, ref)[0, 0].max()) == 0.0  # the other head is untouched


def test_dq_tail_error_hides_under_the_global_bound():
    """30 % on one (b, h)'s 16-row dq tail tile at (B, H, Np) = (2, 2, 1040)."""
    q, k, v = (t.double().requires_grad_(True) for t in attn_inputs(2, 2, 1040, seed=1042))
    out = restate.attend(q, k, v, scale=10.0)
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=out.dtype) * 1e-3)
    ref = q.grad
    got = _confine(ref, 1, 0, slice(1024, 1040), 0.3, seed=2)
    assert rel_err(got, ref) < 2e-2, rel_err(got, ref)  # test_attn_fwd_bwd's dq bound: accepted
    err, idx = worst_tile(tile_errors(got, ref))
    assert idx == (1, 0, 8) and abs(err - 0.3) < 1e-9, (err, idx)
    assert err > BOUNDS["spread"]["dq_tile"]
    # the qk-norm group measures dq tiles against half the typical tile norm (one-hot rows): the error is still rejected there
    err_f, idx_f = worst_tile(tile_errors(got, ref, floor=BOUNDS["qknorm"]["floor"]["dq"]))
    assert idx_f == (1, 0, 8) and err_f > BOUNDS["qknorm"]["dq_tile"], (err_f, idx_f)


def test_tile_errors_zero_reference_tiles():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(2, 3, 300, 64, generator=g, dtype=torch.float64)
    ref[0, 1, 128:256] = 0  # a masked key tile: dk / dv of masked keys are exactly zero
    ref[1] = 0  # a fully masked batch: its dq and dk
    got = ref.clone()
    e = tile_errors(got, ref)
    assert e.shape == (2, 3, 3) and float(e.max()) == 0.0
    got[0, 1, 200, 5] = 1e-30  # the smallest departure from an exactly-zero reference tile is rejected
    e = tile_errors(got, ref)
    assert math.isinf(float(e[0, 1, 1])) and float(e[0, 1, 0]) == 0.0
    got = ref.clone()
    got[1, 2, 299] = -0.0  # signed zero is zero
    assert float(tile_errors(got, ref).max()) == 0.0
    # a NEARLY zero tile is measured against the floor 1e-3 * rms(ref) * sqrt(n): an error far below the floor stays small
    ref2 = ref.clone()
    ref2[0, 0, :128] = 1e-12
    got2 = ref2.clone()
    got2[0, 0, :128] += 1e-12
    e2 = float(tile_errors(got2, ref2)[0, 0, 0])
    assert 0 < e2 < 1e-6, e2
    # the last, partial tile is measured over its own rows (44 here); NaN fails a Checks bound
    got3 = ref.clone()
    got3[0, 0, 256:] *= 1.01
    assert abs(float(tile_errors(got3, ref)[0, 0, 2]) - 0.01) < 1e-12
    got3[0, 2, 7, 7] = math.nan
    chk = Checks("nan")
    chk.tiles("x", got3, ref, 1.0)
    assert chk.bad


def test_tile_errors_lse_axis():
    ref = torch.linspace(1, 2, 2 * 2 * 1029, dtype=torch.float64).view(2, 2, 1029)
    got = ref.clone()
    got[1, 1, 1025] += 1e-2
    e = tile_errors(got, ref, axis=-1)
    assert e.shape == (2, 2, 9)
    assert worst_tile(e)[1] == (1, 1, 8) and float(e[0].max()) == 0.0
