"""fp64 restatement of the LoRA merge and adapter gradients (csrc/lora.hip, include/vbx.h "LoRA adapters"), with the per-element
bound terms of the kernel contracts and a switch for planted faults (tests/test_finetune_cpu.py measures how far each moves a result).

    merge:  W = W0 + s . B . A            s = alpha / r,  A [r, K],  B [N, r]
    grads:  dB = s . dW . A^T             dA = s . B^T . dW           (dW [N, K]: the gradient of the loss with respect to W)
"""
import torch

FAULTS = ("alpha_not_over_r", "swap_ab", "da_from_w", "scale_missing", "transposed")


def scale(alpha, r, fault=None):
    return float(alpha) if fault == "alpha_not_over_r" else float(alpha) / r


def merge(w0, A, B, alpha, fault=None):
    """-> (W, bound term |W0| + |s| sum_j |B A|), fp64.  The faults "swap_ab" and "transposed" need N == K to have a shape."""
    w0, A, B = w0.double(), A.double(), B.double()
    s = scale(alpha, A.shape[0], fault)
    ba = B @ A
    if fault in ("swap_ab", "transposed"):  # A^T where B belongs and B^T where A belongs: the transposed product
        assert w0.shape[0] == w0.shape[1]
        ba = A.t() @ B.t()
    return w0 + s * ba, w0.abs() + abs(s) * (B.abs() @ A.abs())


def grads(dW, A, B, alpha, fault=None, W=None):
    """-> (dA, dB, bound term of dA = |s| sum_n |B dW|, bound term of dB = |s| sum_k |dW A|), fp64"""
    dW, A, B = dW.double(), A.double(), B.double()
    s = scale(alpha, A.shape[0], fault)
    src = W.double() if fault == "da_from_w" else dW
    dA = s * (B.t() @ src)
    dB = (1.0 if fault == "scale_missing" else s) * (dW @ A.t())
    if fault == "swap_ab":  # each gradient by the other one's formula
        assert dW.shape[0] == dW.shape[1]
        dA, dB = (s * (dW @ A.t())).t().contiguous(), (s * (B.t() @ dW)).t().contiguous()
    if fault == "transposed":  # dW read as [K, N]
        assert dW.shape[0] == dW.shape[1]
        dA, dB = s * (B.t() @ dW.t()), s * (dW.t() @ A.t())
    return dA, dB, abs(s) * (B.abs().t() @ dW.abs()), abs(s) * (dW.abs() @ A.abs().t())


U = 2.0 ** -24


def merge_bound(term, r):
    return (r + 2) * U * term


def grad_bounds(term_a, term_b, N, K):
    return (N + 2) * U * term_a, (K + 2) * U * term_b


def fault_movements(seed=7):
    """{fault: the largest relative movement max|faulty - right| / max|right| over (W, dA, dB)} on one fixed square case
    (N = K = 64, r = 4, alpha = 12: alpha differs from alpha / r, and the transposes have a shape)."""
    g = torch.Generator().manual_seed(seed)
    N = K = 64
    r, alpha = 4, 12.0
    w0, dW = torch.randn(N, K, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64)
    A, B = torch.randn(r, K, generator=g, dtype=torch.float64) / K ** 0.5, torch.randn(N, r, generator=g, dtype=torch.float64)
    W, _ = merge(w0, A, B, alpha)
    dA, dB, _, _ = grads(dW, A, B, alpha, W=W)
    out = {}
    for f in FAULTS:
        Wf, _ = merge(w0, A, B, alpha, fault=f)
        dAf, dBf, _, _ = grads(dW, A, B, alpha, fault=f, W=W)
        out[f] = max(float((x - y).abs().max() / y.abs().max()) for x, y in ((Wf, W), (dAf, dA), (dBf, dB)))
    return out


def fault_tolerance():
    """The relative tolerance of the GPU tests: a tenth of the smallest movement a planted fault causes."""
    return min(fault_movements().values()) / 10
