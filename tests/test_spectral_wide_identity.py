"""What the spectral cross op beyond 32 columns computes (csrc/lr_cross_spectral_kernel.hpp), restated in NumPy and held against torch autograd of
autodiff.base_kernel_matrix("spectral", ...): the value from the expanded squared distance xs + ss - 2 ip and the phase difference
phi(p) - phi(s), and the five gradients from A_q = G o alpha_q cos(theta_q) dE_q/dsq and B_q = -2 pi G o alpha_q E_q sin(theta_q):

    dalpha_q   = sum G o E_q cos(theta_q)
    dP         = sum_q [2 gamma_q^2 o (rowsum(A_q) o P - A_q S) + omega_q (x) rowsum(B_q)]
    dS         = sum_q [2 gamma_q^2 o (colsum(A_q) o S - A_q^T P) - omega_q (x) colsum(B_q)]
    domega_qf  = sum_t rowsum(B_q)_t p_tf - sum_i colsum(B_q)_i s_if
    dgamma_qf  = 2 gamma_qf [sum_t rowsum(A_q)_t p_tf^2 + sum_i colsum(A_q)_i s_if^2 - 2 sum_i s_if (A_q^T P)_if]

On the grid data of tests/test_gpu_lowrank_spectral_wide.py (points on 1/256, parameters on 1/8, half the landmarks copied from points) at
(n, c, d, Q) = (16, 17, 65, 3); relerr <= 1e-12.  No GPU; it passes with or without the op."""
import numpy as np
import pytest
import torch

from gpsig_amd import autodiff

FAMILIES = ("rbf", "exp", "mixed")


def grid(a, step=256.0):
    return np.clip(np.round(np.asarray(a) * step) / step, -7.0, 7.0)


def data(n, c, d, Q, seed):
    rng = np.random.default_rng(seed)
    P = grid(rng.standard_normal((n, d)) * 1.5 / np.sqrt(d))
    S = grid(rng.standard_normal((c, d)) * 1.5 / np.sqrt(d))
    take = rng.choice(n, min((c + 1) // 2, n), replace=False)
    S[: len(take)] = P[take]
    alpha = rng.uniform(0.3, 1.2, Q)
    omega = np.round(rng.uniform(-1.0, 1.0, (Q, d)) * 8.0) / 8.0
    gamma = np.round(rng.uniform(0.5, 1.5, (Q, d)) * 8.0) / 8.0
    return P, S, alpha, omega, gamma


def restated(P, S, alpha, omega, gamma, family, G):
    Q = alpha.shape[0]
    K = np.zeros((P.shape[0], S.shape[0]))
    dP, dS, dal, dom, dga = np.zeros_like(P), np.zeros_like(S), np.zeros_like(alpha), np.zeros_like(omega), np.zeros_like(gamma)
    for q in range(Q):
        g2 = gamma[q] ** 2
        ip, xs, ss = (P * g2) @ S.T, ((P * g2) * P).sum(1), ((S * g2) * S).sum(1)
        sq = np.maximum(xs[:, None] + ss[None, :] - 2.0 * ip, 0.0)
        th = 2.0 * np.pi * ((P @ omega[q])[:, None] - (S @ omega[q])[None, :])
        if family == "rbf" or (family == "mixed" and q < Q // 2):
            E = np.exp(-sq / 2)
            dE = -E / 2
        else:
            s = np.sqrt(sq)
            E = np.exp(-s / 2)
            dE = np.where(s > 0, -E / (4 * np.where(s > 0, s, 1.0)), 0.0)
        K += alpha[q] * E * np.cos(th)
        A = G * alpha[q] * np.cos(th) * dE
        B = -2.0 * np.pi * G * alpha[q] * E * np.sin(th)
        AtP = A.T @ P
        dal[q] = (G * E * np.cos(th)).sum()
        dP += 2.0 * g2 * (A.sum(1)[:, None] * P - A @ S) + np.outer(B.sum(1), omega[q])
        dS += 2.0 * g2 * (A.sum(0)[:, None] * S - AtP) - np.outer(B.sum(0), omega[q])
        dom[q] = B.sum(1) @ P - B.sum(0) @ S
        dga[q] = 2.0 * gamma[q] * (A.sum(1) @ P ** 2 + A.sum(0) @ S ** 2 - 2.0 * (S * AtP).sum(0))
    return K, (dP, dS, dal, dom, dga)


def relerr(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


@pytest.mark.parametrize("family", FAMILIES)
def test_the_restated_formulas_match_autograd(family):
    n, c, d, Q = 16, 17, 65, 3
    arrays = data(n, c, d, Q, seed=n + c + d + Q)
    G = np.random.default_rng(3).standard_normal((n, c))
    leaves = [torch.tensor(a, requires_grad=True) for a in arrays]
    P, S, al, om, ga = leaves
    want = autodiff.base_kernel_matrix("spectral", P, S, spectral=(family, al, om, ga))
    want_g = torch.autograd.grad(want, leaves, torch.tensor(G))
    K, grads = restated(*arrays, family, G)
    e = relerr(K, want.detach().numpy())
    print("values", family, e)
    assert e <= 1e-12, e
    for name, g, w in zip(("dP", "dS", "dalpha", "domega", "dgamma"), grads, want_g):
        assert np.isfinite(g).all()
        e = relerr(g, w.numpy())
        print("gradient", family, name, e)
        assert e <= 1e-12, (name, e)
