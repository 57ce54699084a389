"""A host reference of the Nystrom cross ops, plain numpy in np.longdouble (80-bit on x86; where longdouble is no wider than double it is
still an independent reference): what gpsig_lr_cross / gpsig_lr_cross_grad and gpsig_spectral_cross / gpsig_spectral_cross_grad compute, for the
GPU tests of their loops and edges (tests/test_gpu_cross_edges.py).  tests/test_cross_reference.py checks it against
autodiff.base_kernel_matrix under torch autograd on the CPU.

cross / cross_grad: the eight families of base_kernel_matrix as closed forms in ip = P S^T, |P|^2 and |S|^2 -- no autograd, no (n, c, d) tensor:
    dP = (G o (k_ip - 2 k_dist)) S + 2 rowsum(G o (k_xs + k_dist)) o P,    dS likewise with the transposes and the column sums,
with k_ip, k_xs, k_ss, k_dist the partial derivatives of kappa in the inner product, the two squared norms and dist = xs + ss - 2 ip.  The Matern
families clamp dist at 1e-40 before the root, so nothing flows through a zero distance.

spectral_cross / spectral_cross_grad: on the difference tensor, as base_kernel_matrix("spectral", ...), in blocks of rows of at most BLOCK_ELEMS
elements of it (a handful of longdouble temporaries of that size: below 200 MB); the root of the exponential envelope has derivative 0 at 0
(autodiff._SqrtZeroGrad)."""
import math

import numpy as np

LD = np.longdouble
FAMILIES = ("linear", "cosine", "poly", "rbf", "mix", "matern12", "matern32", "matern52")
SPECTRAL_FAMILIES = ("rbf", "exp", "mixed")
BLOCK_ELEMS = 1 << 20                                      # (16 MB a temporary)
TWO_PI = LD(2.0 * math.pi)                                  # (the double the kernels and torch multiply with)


def _ld(a):
    return np.asarray(a, dtype=LD)


def _partials(base, ip, xs, ss, p0, p1, grad):
    """kappa and, with ``grad``, (k_ip, k_xs, k_ss, k_dist, k_p0) -- None where a family has no such term"""
    p0, p1 = LD(p0), LD(p1)
    if base == "linear":
        return ip, (np.ones_like(ip), None, None, None, None)
    if base == "cosine":
        den = np.sqrt(xs)[:, None] * np.sqrt(ss)[None, :]
        k = ip / den
        return k, ((1 / den, -k / (2 * xs[:, None]), -k / (2 * ss[None, :]), None, None) if grad else None)
    if base == "poly":
        b = ip + p0
        k = b ** p1
        dk = p1 * b ** (p1 - 1)
        return k, (dk, None, None, None, dk)
    dist = xs[:, None] + ss[None, :] - 2 * ip
    if base == "rbf":
        k = np.exp(-dist / 2)
        return k, (None, None, None, -k / 2, None)
    if base == "mix":
        e = np.exp(-dist / 2)
        return p0 * e + (1 - p0) * ip, (np.full_like(ip, 1 - p0), None, None, -p0 * e / 2, e - ip)
    free = dist > LD(1e-40)
    r = np.sqrt(np.maximum(dist, LD(1e-40)))
    if base == "matern12":
        k = np.exp(-r)
        k_r = -k
    elif base == "matern32":
        s = np.sqrt(LD(3))
        e = np.exp(-s * r)
        k = (1 + s * r) * e
        k_r = -3 * r * e
    elif base == "matern52":
        s = np.sqrt(LD(5))
        e = np.exp(-s * r)
        k = (1 + s * r + LD(5) / 3 * r * r) * e
        k_r = -(LD(5) / 3) * r * (1 + s * r) * e
    else:
        raise ValueError(base)
    return k, (None, None, None, np.where(free, k_r / (2 * r), 0), None)


def _operands(P, S):
    P, S = _ld(P), _ld(S)
    return P, S, P @ S.T, (P * P).sum(1), (S * S).sum(1)


def cross(base, P, S, p0=0.0, p1=0.0):
    """kappa(P_t, S_i) of base_kernel_matrix(base, P, S, p0, p1): (n, d), (c, d) -> (n, c) longdouble"""
    P, S, ip, xs, ss = _operands(P, S)
    return _partials(base, ip, xs, ss, p0, p1, False)[0]


def cross_grad(base, P, S, G, p0=0.0, p1=0.0):
    """the reverse pass of ``cross`` for dL/dK = G (n, c) -> (dP, dS, g_base); g_base = dL/dp0, 0 for the families without a p0"""
    P, S, ip, xs, ss = _operands(P, S)
    G = _ld(G)
    k_ip, k_xs, k_ss, k_dist, k_p0 = _partials(base, ip, xs, ss, p0, p1, True)[1]
    zero = np.zeros_like(ip)
    A = G * ((zero if k_ip is None else k_ip) - 2 * (zero if k_dist is None else k_dist))
    ax = (G * ((zero if k_xs is None else k_xs) + (zero if k_dist is None else k_dist))).sum(1)
    cs = (G * ((zero if k_ss is None else k_ss) + (zero if k_dist is None else k_dist))).sum(0)
    dP = A @ S + 2 * ax[:, None] * P
    dS = A.T @ P + 2 * cs[:, None] * S
    return dP, dS, (LD(0) if k_p0 is None else (G * k_p0).sum())


def _gauss(family, q, Q):
    if family not in SPECTRAL_FAMILIES:
        raise ValueError(family)
    return family == "rbf" or (family == "mixed" and q < Q // 2)


def _blocks(n, c, d):
    rows = max(1, BLOCK_ELEMS // max(1, c * d))
    return [(t, min(n, t + rows)) for t in range(0, n, rows)]


def _component(family, q, Q, diff, omega, gamma, grad):
    """the envelope E, its derivative in the squared scaled distance, and the cosine and sine of the phase, of one component on one block"""
    sq = np.square(diff * gamma[q]).sum(-1)
    if _gauss(family, q, Q):
        E = np.exp(-sq / 2)
        E_sq = -E / 2
    else:
        root = np.sqrt(sq)
        E = np.exp(-root / 2)
        E_sq = np.where(root > 0, -E / (4 * np.where(root > 0, root, 1)), 0) if grad else None
    ph = TWO_PI * (diff * omega[q]).sum(-1)
    return E, E_sq, np.cos(ph), (np.sin(ph) if grad else None)


def spectral_cross(family, P, S, alpha, omega, gamma):
    """base_kernel_matrix("spectral", P, S, spectral=(family, alpha, omega, gamma)): (n, d), (c, d), (Q,), (Q, d), (Q, d) -> (n, c) longdouble"""
    P, S, alpha, omega, gamma = (_ld(a) for a in (P, S, alpha, omega, gamma))
    (n, d), c, Q = P.shape, S.shape[0], alpha.shape[0]
    K = np.zeros((n, c), dtype=LD)
    for t0, t1 in _blocks(n, c, d):
        diff = P[t0:t1, None, :] - S[None, :, :]
        for q in range(Q):
            E, _, C, _ = _component(family, q, Q, diff, omega, gamma, False)
            K[t0:t1] += alpha[q] * E * C
    return K


def spectral_cross_grad(family, P, S, alpha, omega, gamma, G):
    """the reverse pass of ``spectral_cross`` for dL/dK = G -> (dP, dS, dalpha, domega, dgamma)"""
    P, S, alpha, omega, gamma, G = (_ld(a) for a in (P, S, alpha, omega, gamma, G))
    (n, d), c, Q = P.shape, S.shape[0], alpha.shape[0]
    dP, dS = np.zeros_like(P), np.zeros_like(S)
    dal, dom, dga = np.zeros_like(alpha), np.zeros_like(omega), np.zeros_like(gamma)
    for t0, t1 in _blocks(n, c, d):
        diff = P[t0:t1, None, :] - S[None, :, :]
        ddiff = np.zeros_like(diff)
        Gb = G[t0:t1]
        for q in range(Q):
            E, E_sq, C, Sn = _component(family, q, Q, diff, omega, gamma, True)
            dal[q] += (Gb * E * C).sum()
            w_sq = Gb * alpha[q] * C * E_sq                 # dL / d sq_q
            w_u = -Gb * alpha[q] * E * Sn * TWO_PI          # dL / d (diff . omega_q)
            t = w_sq[:, :, None] * diff                     # (one temporary of the block's size)
            dga[q] += 2 * gamma[q] * (t * diff).sum((0, 1))
            ddiff += 2 * np.square(gamma[q]) * t
            dom[q] += (w_u[:, :, None] * diff).sum((0, 1))
            ddiff += w_u[:, :, None] * omega[q]
        dP[t0:t1] = ddiff.sum(1)
        dS -= ddiff.sum(0)
    return dP, dS, dal, dom, dga
