"""CPU side of the aligner primitives (maximum_path / forward_sum_loss): the fp64 restatements of tests/align_ref.py against a
brute force over all monotonic paths and against F.ctc_loss, planted faults that the checks of tests/test_align_gpu.py must
catch on that test's own inputs, and the refusals of the public calls."""
import pytest
import torch

import align_ref as ar


# ----------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("T,K", [(6, 3), (9, 4), (7, 7), (8, 1)])
def test_path_restatement_is_the_brute_force_optimum_with_stay_on_tie(T, K):
    ties = 0
    for seed in range(12):
        g = torch.Generator().manual_seed(100 * T + seed)
        v = torch.randint(-1, 2, (T, K), generator=g).float()  # three values: most optima are shared by several paths
        path, dur, Q = ar.maximum_path_ref(v, T, K)
        want, best = ar.brute_force_path(v, T, K)
        assert torch.equal(path, want), (seed, path, want)
        assert float(Q[T - 1, K - 1]) == best and torch.equal(dur, want.sum(0).long())
        ties += not torch.equal(path, ar.maximum_path_ref(v, T, K, "tie_moves")[0])
        if T > K and K > 1:  # shorter lengths inside a larger map
            path, _, _ = ar.maximum_path_ref(v, T - 1, K - 1)
            want, _ = ar.brute_force_path(v[:T - 1, :K - 1], T - 1, K - 1)
            assert torch.equal(path[:T - 1, :K - 1], want) and not bool(path[T - 1:].any()) and not bool(path[:, K - 1:].any())
    assert ties > 0 or K in (1, T)  # the inputs do exercise the tie rule wherever a path has a choice


def mixed_batch(dtype):
    g = torch.Generator().manual_seed(5)
    x = (3.0 * torch.randn(4, 12, 5, generator=g)).to(dtype)
    return x, [5, 3, 5, 5], [12, 12, 8, 4]  # full, key_len < K, query_len < T, infeasible


def test_loss_restatement_is_ctc_loss_in_fp64():
    x, klens, qlens = mixed_batch(torch.float64)
    for reduction in ("mean", "none"):
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        mine = ar.forward_sum_ref(a, klens, qlens, -1.0, reduction)
        theirs = ar.ctc_construction(b, klens, qlens, -1.0, reduction)
        assert float((mine - theirs).detach().abs().max()) <= 1e-12, (reduction, mine, theirs)
        ga, = torch.autograd.grad(mine.sum(), a)
        gb, = torch.autograd.grad(theirs.sum(), b)
        assert float((ga - gb).abs().max()) <= 1e-12
        assert not bool(ga[3].any()) and not bool(ga[1, :, 3:].any()) and not bool(ga[2, 8:].any())
    assert float(ar.forward_sum_ref(x, klens, qlens, reduction="none")[3]) == 0.0


# ----------------------------------------------------------------------------- planted faults, on the GPU test's inputs
LOSS_SHAPE = (3, 70, 65)
PATH_SHAPES = [(3, 7, 7), (3, 70, 65), (3, 65, 9)]


@pytest.mark.parametrize("fault", ar.LOSS_FAULTS)
def test_planted_loss_faults_exceed_ten_times_the_gpu_tolerance(fault):
    """the tolerance is the one tests/test_align_gpu.py computes on these inputs; the ratio is a condition on the inputs"""
    B, T, K = LOSS_SHAPE
    moved = {}
    for batch in range(len(ar.length_batches(B, T, K))):
        ref = ar.loss_reference(B, T, K, batch)
        tol = ar.loss_tolerances(ref, T)
        x = ref["x"].double()
        nll = ar.forward_sum_ref(x, ref["klens"], ref["qlens"], -1.0, "none", fault)
        mean = ar.forward_sum_ref(x, ref["klens"], ref["qlens"], -1.0, "mean", fault)
        moved[batch] = max(float(((nll - ref["nll"]).abs() / tol["nll"]).max()), abs(float(mean - ref["mean"])) / tol["mean"])
    print(fault, moved)
    assert max(moved.values()) >= 10.0, moved


@pytest.mark.parametrize("fault", ar.PATH_FAULTS)
def test_planted_path_faults_break_bit_equality_on_the_integer_inputs(fault):
    """test (a) of the GPU file asks for bit-equal paths on integer scores: its tolerance is 0, any changed cell is caught"""
    changed, refused = 0, 0
    for B, T, K in PATH_SHAPES:
        for batch in range(len(ar.length_batches(B, T, K))):
            value, qlens, klens, path, dur, _, _ = ar.path_reference("int", B, T, K, batch)
            bad, bad_dur, _, _ = ar.maximum_path_batch_ref(value, qlens, klens, fault)
            changed += int((bad != path).sum())
            refused += bool(ar.path_problems(bad, bad_dur, qlens, klens))
    assert changed > 0, fault
    assert refused > 0 or fault != "start_at_K"  # the wrong last key is also what the validity check of test (b) refuses


def test_path_checker_accepts_the_restatement_and_the_bound_holds_for_an_fp32_table():
    B, T, K = 3, 70, 65
    value, qlens, klens, path, dur, best, qmax = ar.path_reference("gauss", B, T, K, 0)
    assert ar.path_problems(path, dur, qlens, klens) == []
    score = ar.path_score(path, value)
    for b in range(B):
        if best[b] is not None:
            assert abs(float(score[b]) - best[b]) <= 1e-9 * max(1.0, abs(best[b]))
    wrong = path.clone()
    wrong[0, 10] = wrong[0, 10].flip(0)
    assert ar.path_problems(wrong, dur, qlens, klens)


def test_every_batch_set_covers_the_six_kinds_of_row():
    for B, T, K in ar.SHAPES:
        rows = {(q, k) for ql, kl in ar.length_batches(B, T, K) for q, k in zip(ql, kl)}
        assert any(q == T and k == K for q, k in rows)
        assert any(k < K and q >= k for q, k in rows) or K == 1
        assert any(q < T and q >= k for q, k in rows)
        assert any(q == k for q, k in rows) and any(q == k + 1 for q, k in rows)
        assert any(q < k for q, k in rows)
        for ql, kl in ar.length_batches(B, T, K):
            assert len(ql) == B and all(0 <= q <= T and 1 <= k <= K for q, k in zip(ql, kl))


# ----------------------------------------------------------------------------- refusals
def test_cpu_tensors_raise_no_cpu_fallback():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    x = torch.zeros(2, 6, 3)
    lens = torch.tensor([3, 2])
    for call in (lambda: vbx.maximum_path(x), lambda: vbx.maximum_path(x[:, None], torch.tensor([6, 5]), lens),
                 lambda: vbx.forward_sum_loss(x, lens, torch.tensor([6, 5])), lambda: vbx.forward_sum_loss(x, reduction="none"),
                 lambda: vbx.ForwardSumLoss()(x[:, None], lens, torch.tensor([6, 5]))):
        with pytest.raises(_lib.VbxError, match="no CPU fallback"):
            call()
    assert vbx.ForwardSumLoss().blank_logprob == -1.0 and vbx.ForwardSumLoss(blank_logprob=-2.0).blank_logprob == -2.0


def test_too_many_keys_raise_before_any_launch():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    x = torch.zeros(1, 2, 1025)
    with pytest.raises(NotImplementedError, match="1024"):
        vbx.maximum_path(x)
    with pytest.raises(NotImplementedError, match="1024"):
        vbx.forward_sum_loss(x)
    l = _lib.lib()
    p = 4096  # a placeholder pointer: the arguments are validated on the host first
    assert l.vbx_maximum_path(p, None, None, p, p, p, 1, 2, 1025, None) != 0 and b"1 .. 1024" in l.vbx_last_error()
    assert l.vbx_forward_sum_fwd(p, None, None, -1.0, p, p, p, p, 1, 2, 1025, None) != 0 and b"1 .. 1024" in l.vbx_last_error()
    assert l.vbx_forward_sum_bwd(p, None, None, -1.0, p, p, p, p, p, 1, 0, 4, None) != 0 and b"T >= 1" in l.vbx_last_error()
    assert l.vbx_maximum_path(None, None, None, p, p, p, 1, 2, 4, None) != 0 and b"null operand" in l.vbx_last_error()


def test_shape_and_dtype_errors_raise_value_error():
    import voicebox_pytorch_amd as vbx

    x = torch.zeros(2, 6, 3)
    for bad in (torch.zeros(6, 3), torch.zeros(2, 2, 6, 3), torch.zeros(2, 6, 3, dtype=torch.int64), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError):
            vbx.maximum_path(bad)
        with pytest.raises(ValueError):
            vbx.forward_sum_loss(bad)
    for lens in (torch.tensor([3.0, 2.0]), torch.tensor([3, 2, 1]), torch.tensor([[3, 2]]), [3, 2]):
        with pytest.raises(ValueError):
            vbx.maximum_path(x, lens, None)
        with pytest.raises(ValueError):
            vbx.forward_sum_loss(x, lens, None)
        with pytest.raises(ValueError):
            vbx.forward_sum_loss(x, None, lens)
    with pytest.raises(ValueError, match="reduction"):
        vbx.forward_sum_loss(x, reduction="sum")
    with pytest.raises(ValueError, match="finite"):
        vbx.forward_sum_loss(x, blank_logprob=float("-inf"))
