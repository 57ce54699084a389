"""The batched SignatureSpectral kappa op, its two C entry points called directly: gpsig_spectral_kappa / gpsig_spectral_kappa_grad
(csrc/spectral_kappa_api.hip; forward: the kernels of csrc/wide_spectral_kernel.hpp, reverse: csrc/spectral_kappa_kernel.hpp).

Reference: autodiff.base_kernel_matrix("spectral", ...) in float64 on the device -- the difference form -- with torch autograd for the five gradients.
Errors are max|got - want| / max|want| per array; bounds: 1e-10 for values (tests/test_gpu_wide_spectral.py), 1e-9 for gradients (tests/test_gpu_wide.py).
Inputs 0.7 * randn; alpha in U(0.3, 1.2), omega in U(0.05, 0.3) / sqrt(d), gamma in U(0.4, 1.3) / sqrt(d) -- positive, and scaled so that the squared
distances stay of order one at every width (at d = 4096 unscaled parameters underflow every entry to 0 and the comparison would be empty).

Errors measured on the GPU (MI355X), the largest over the cases of each test:
    values and all five gradients, 13 cases: values 0 .. 1.9e-15 (5.0e-15 at d = 4,096), gradients 1.1e-16 .. 2.7e-15 (the largest at d = 4,096;
        1.7e-15 below it: dalpha at Q = 17)
    self-pairs: one array on both sides 4.5e-16 / 8.1e-16, copied rows 4.5e-16 / 9.8e-16; the self-pair entries equal sum(alpha) bit for bit
    chunks: wide_chunk_mb = 1 and the default 7.0e-16 / 8.3e-16 each (row chunks), 5.4e-16 / 6.9e-16 (chunks of batch members), the same bits on repeat
    memory: the allocator's peak rose by 100.0 MiB
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_VALUE, TOL_GRAD = 1e-10, 1e-9
FAMILY = {"rbf": 0, "exp": 1, "mixed": 2}

# (batch, m, n), d, Q, family: every shape, width, number of components and family of the list at least once; Q = 17 'mixed' is the odd split
CASES = [
    ((1, 1, 1), 1, 1, "rbf"),
    ((1, 16, 17), 4, 5, "exp"),
    ((1, 63, 65), 31, 16, "mixed"),
    ((1, 64, 64), 33, 17, "mixed"),
    ((3, 65, 63), 63, 5, "rbf"),
    ((2, 130, 70), 65, 64, "exp"),
    ((2, 130, 70), 130, 1, "rbf"),
    ((1, 63, 65), 130, 5, "exp"),
    ((3, 65, 63), 4, 17, "rbf"),
    ((1, 16, 17), 33, 64, "rbf"),
    ((1, 64, 64), 63, 16, "exp"),
    ((1, 1, 1), 31, 5, "mixed"),
    ((1, 16, 16), 4096, 2, "rbf"),
]


def rel(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))


def ctx():
    from gpsig_amd import _lib
    c = _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream)
    c.set_pointer_mode(_lib.PTR_DEVICE)
    return c


def ptr(t):
    return C.c_void_p(t.data_ptr())


def data(seed, batch, m, n, d, Q):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float64)
    A, B, G = 0.7 * rn(batch, m, d), 0.7 * rn(batch, n, d), rn(batch, m, n)
    alpha, omega, gamma = ru(0.3, 1.2, Q), ru(0.05, 0.3, Q, d) / d ** 0.5, ru(0.4, 1.3, Q, d) / d ** 0.5
    return tuple(t.to(DEV) for t in (A, B, G, alpha, omega, gamma))


def kappa(A, B, alpha, omega, gamma, family):
    batch, m, d = A.shape
    n, Q = B.shape[1], alpha.shape[0]
    K = torch.full((batch, m, n), float("nan"), dtype=torch.float64, device=DEV)
    c = ctx()
    c.check(c._lib.gpsig_spectral_kappa(c._h, Q, FAMILY[family], d, ptr(A), ptr(B), batch, m, n, ptr(alpha), ptr(omega), ptr(gamma), ptr(K)))
    return K


def kappa_grad(A, B, alpha, omega, gamma, family, G):
    batch, m, d = A.shape
    n, Q = B.shape[1], alpha.shape[0]
    outs = tuple(torch.full(s, float("nan"), dtype=torch.float64, device=DEV) for s in ((batch, m, d), (batch, n, d), (Q,), (Q, d), (Q, d)))
    c = ctx()
    c.check(c._lib.gpsig_spectral_kappa_grad(c._h, Q, FAMILY[family], d, ptr(A), ptr(B), batch, m, n, ptr(alpha), ptr(omega), ptr(gamma), ptr(G),
                                             *(ptr(o) for o in outs)))
    return outs


def reference(A, B, alpha, omega, gamma, family, G, same=False):
    """K and the five gradients by the difference form under autograd; same: B IS A (one leaf, whose gradient is the sum of both sides')"""
    from gpsig_amd.autodiff import base_kernel_matrix
    leaves = [t.clone().requires_grad_(True) for t in ((A, alpha, omega, gamma) if same else (A, B, alpha, omega, gamma))]
    a, b = (leaves[0], leaves[0]) if same else leaves[:2]
    K = base_kernel_matrix("spectral", a, b, spectral=(family,) + tuple(leaves[-3:]))
    (K * G).sum().backward()
    return K.detach(), [t.grad for t in leaves]


def check(tag, K, grads, Kw, gw):
    errs = [rel(K, Kw)] + [rel(g, w) for g, w in zip(grads, gw)]
    print(tag, "value %.1e" % errs[0], "gradients", " ".join("%.1e" % e for e in errs[1:]))
    assert all(bool(torch.isfinite(g).all()) for g in grads), tag
    assert errs[0] < TOL_VALUE, (tag, errs)
    assert max(errs[1:]) < TOL_GRAD, (tag, errs)


@pytest.mark.parametrize("shape,d,Q,family", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_values_and_all_five_gradients(shape, d, Q, family):
    A, B, G, alpha, omega, gamma = data(11, *shape, d, Q)
    K = kappa(A, B, alpha, omega, gamma, family)
    grads = kappa_grad(A, B, alpha, omega, gamma, family, G)
    Kw, gw = reference(A, B, alpha, omega, gamma, family, G)
    check("%s d=%d Q=%d %s:" % (shape, d, Q, family), K, grads, Kw, gw)


def ordered_sum(alpha):
    s = 0.0
    for a in alpha.cpu().tolist():
        s += a
    return s


def test_self_pairs_one_array_on_both_sides():
    """A and B are ONE array ('exp': the square root at zero distance): the diagonal is sum(alpha) exactly, dA + dB is the reference's gradient"""
    A, _, G, alpha, omega, gamma = data(12, 2, 70, 70, 63, 5)
    K = kappa(A, A, alpha, omega, gamma, "exp")
    dA, dB, da, do, dg = kappa_grad(A, A, alpha, omega, gamma, "exp", G)
    diag = torch.diagonal(K, dim1=1, dim2=2)
    assert bool((diag == ordered_sum(alpha)).all()), float((diag - ordered_sum(alpha)).abs().max())
    Kw, gw = reference(A, None, alpha, omega, gamma, "exp", G, same=True)
    check("self-pairs, one array:", K, [dA + dB, da, do, dg], Kw, gw)


def test_self_pairs_copied_rows():
    """B holds bitwise copies of a few rows of A"""
    A, B, G, alpha, omega, gamma = data(13, 2, 70, 70, 63, 5)
    rows_a, rows_b = [5, 60, 69, 0], [3, 10, 64, 69]
    B[:, rows_b] = A[:, rows_a]
    K = kappa(A, B, alpha, omega, gamma, "exp")
    assert bool((K[:, rows_a, rows_b] == ordered_sum(alpha)).all())
    grads = kappa_grad(A, B, alpha, omega, gamma, "exp", G)
    Kw, gw = reference(A, B, alpha, omega, gamma, "exp", G)
    check("self-pairs, copied rows:", K, grads, Kw, gw)


@pytest.mark.parametrize("batch,m,n", [(1, 300, 130), (7, 33, 31)])
def test_chunks(batch, m, n):
    """wide_chunk_mb = 1 -- several row chunks of one member (300 x 130: U alone is 1.5 MB; a 64-row block takes 0.74 MB, two do not fit), chunks of
    several whole members (seven of 33 x 31, about 0.24 MB of scratch each: four, then three) -- and the default budget: both within the bounds, each
    repeating bit for bit.  That the small budget DID chunk is read off the scratch: each setting runs on a context of its own (a fresh stream), whose
    scratch after the calls is the op's one block -- inside the budget (plus the allocator's eighth) under 1 MB, beyond it under the default."""
    A, B, G, alpha, omega, gamma = data(14, batch, m, n, 63, 5)
    Kw, gw = reference(A, B, alpha, omega, gamma, "mixed", G)
    limit = 2 ** 20 + 2 ** 20 // 8 + 1024                      # the budget, ensure()'s headroom of an eighth + 256 bytes, and the block's own 64
    torch.cuda.synchronize()
    for mb in (1, 0):
        with torch.cuda.stream(torch.cuda.Stream(DEV)):
            c = ctx()
            before = c._lib.gpsig_scratch_bytes(c._h)
            c.set_option("wide_chunk_mb", mb)
            try:
                runs = [(kappa(A, B, alpha, omega, gamma, "mixed"),) + kappa_grad(A, B, alpha, omega, gamma, "mixed", G) for _ in range(2)]
                torch.cuda.synchronize()
            finally:
                c.set_option("wide_chunk_mb", 0)
            grown = c._lib.gpsig_scratch_bytes(c._h) - before
        print("wide_chunk_mb = %d: scratch %d bytes" % (mb, grown))
        assert (0 < grown <= limit) if mb else grown > limit, (mb, grown, limit)
        check("wide_chunk_mb = %d:" % mb, runs[0][0], runs[0][1:], Kw, gw)
        for x, y in zip(*runs):
            assert torch.equal(x, y)


@pytest.mark.parametrize("batch,m,n", [(0, 5, 7), (2, 0, 7), (2, 5, 0)])
def test_degenerate_shapes(batch, m, n):
    A, B, G, alpha, omega, gamma = data(15, batch, m, n, 33, 3)
    assert kappa(A, B, alpha, omega, gamma, "rbf").shape == (batch, m, n)
    dA, dB, da, do, dg = kappa_grad(A, B, alpha, omega, gamma, "rbf", G)
    for t in (dA, dB, da, do, dg):
        assert bool((t == 0).all())


def test_refusals():
    """the typed error with the bound in its text; gpsig_spectral_cross keeps its own"""
    from gpsig_amd.autodiff import _SpectralCross
    for d, Q, bound in ((33, 65, "64"), (4097, 2, "4096")):
        A, B, G, alpha, omega, gamma = data(16, 1, 3, 3, d, Q)
        with pytest.raises(NotImplementedError, match=bound):
            kappa(A, B, alpha, omega, gamma, "rbf")
        with pytest.raises(NotImplementedError, match=bound):
            kappa_grad(A, B, alpha, omega, gamma, "rbf", G)
    A, B, G, alpha, omega, gamma = data(16, 1, 9, 65, 33, 2)
    with pytest.raises(NotImplementedError, match="64"):
        _SpectralCross.apply(A[0], B[0], alpha, omega, gamma, "rbf")


def test_memory_through_the_autograd_op():
    """m = n = 2048, d = 64, Q = 5: the difference tensor alone would be 2 GiB; inputs, K, G and the gradients are about 100 MB"""
    from gpsig_amd.autodiff import _SpectralKappa
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    A, B, G, alpha, omega, gamma = data(17, 1, 2048, 2048, 64, 5)
    leaves = [t.requires_grad_(True) for t in (A[0], B[0], alpha, omega, gamma)]
    K = _SpectralKappa.apply(*leaves, "exp")
    (K * G[0]).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    print("allocator peak rose by %.1f MiB" % (rise / 2 ** 20))
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in leaves)
    assert rise < 256 * 2 ** 20, rise
