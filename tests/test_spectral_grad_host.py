"""Host check of gpsig_amd/csrc/spectral_pair.hpp, the per-pair arithmetic of SignatureSpectral's state-space kernel that the low-rank
feature kernels and the spectral cross op (gpsig_spectral_cross / _grad) run: its value against a NumPy restatement of
gpsig/kernels.py:921-942, its gradient (point, landmark, alpha, omega, gamma) against central differences, and the zero-distance
convention of the exponential envelope (derivative of sqrt at 0 taken as 0: finite everywhere)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"rbf": 0, "exp": 1, "mixed": 2}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("spectral") / "libspectral_grad_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "gpsig_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "emu", "spectral_grad_host.cpp")])
    h = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    h.sp_value.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp]
    h.sp_value.restype = C.c_double
    h.sp_grad.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp]
    h.sp_grad.restype = C.c_double
    return h


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _numpy_kappa(alpha, omega, gamma, family, x, y):
    Q = alpha.shape[0]
    diff = x - y
    out = 0.0
    for q in range(Q):
        sq = np.sum((gamma[q] * diff) ** 2)
        gauss = family == "rbf" or (family == "mixed" and q < Q // 2)
        env = np.exp(-sq / 2) if gauss else np.exp(-np.sqrt(sq) / 2)
        out += alpha[q] * env * np.cos(2 * np.pi * np.dot(omega[q], diff))
    return out


class _Pair:
    def __init__(self, lib, Q, d, family, rng, same=False):
        self.lib, self.Q, self.d, self.fam = lib, Q, d, family
        self.alpha = np.exp(rng.standard_normal(Q))
        # frequencies and scales of a size that keeps every term of the sum O(1) at d = 32
        self.omega = np.exp(rng.standard_normal((Q, d))) / d
        self.gamma = np.exp(rng.standard_normal((Q, d))) / np.sqrt(d)
        self.x = rng.standard_normal(d)
        self.y = self.x.copy() if same else rng.standard_normal(d)

    def value(self, alpha=None, omega=None, gamma=None, x=None, y=None):
        a = [np.ascontiguousarray(v if v is not None else w, dtype=np.float64)
             for v, w in ((alpha, self.alpha), (omega, self.omega), (gamma, self.gamma), (x, self.x), (y, self.y))]
        return self.lib.sp_value(_p(a[0]), _p(a[1]), _p(a[2]), self.Q, FAMILIES[self.fam], self.d, _p(a[3]), _p(a[4]))

    def grad(self):
        Q, d = self.Q, self.d
        out = [np.zeros(d), np.zeros(d), np.zeros(Q), np.zeros((Q, d)), np.zeros((Q, d))]
        v = self.lib.sp_grad(_p(self.alpha), _p(self.omega), _p(self.gamma), Q, FAMILIES[self.fam], d, _p(self.x), _p(self.y),
                             *[_p(o) for o in out])
        return v, dict(zip(("x", "y", "alpha", "omega", "gamma"), out))

    def central(self, name, h=1e-6):
        base = getattr(self, name)
        g = np.zeros_like(base)
        for idx in np.ndindex(base.shape):
            up, dn = base.copy(), base.copy()
            up[idx] += h
            dn[idx] -= h
            g[idx] = (self.value(**{name: up}) - self.value(**{name: dn})) / (2 * h)
        return g


@pytest.mark.parametrize("family", ["rbf", "exp", "mixed"])
@pytest.mark.parametrize("Q", [4, 5])
@pytest.mark.parametrize("d", [1, 6, 32])
def test_spectral_pair_value_and_gradient(lib, family, Q, d):
    rng = np.random.default_rng(100 * Q + d + 7 * FAMILIES[family])
    P = _Pair(lib, Q, d, family, rng)
    want = _numpy_kappa(P.alpha, P.omega, P.gamma, family, P.x, P.y)
    v, g = P.grad()
    assert abs(P.value() - want) <= 1e-13 * max(1.0, abs(want))
    assert v == P.value()
    for name in ("x", "y", "alpha", "omega", "gamma"):
        fd = P.central(name)
        scale = max(np.abs(fd).max(), 1e-3)
        err = np.abs(g[name] - fd).max() / scale
        assert err < 1e-6, (name, err)


@pytest.mark.parametrize("family", ["rbf", "exp", "mixed"])
@pytest.mark.parametrize("d", [1, 6, 32])
def test_spectral_pair_zero_distance(lib, family, d):
    """x == y: value sum(alpha); every derivative finite.  By x and y the derivative is 0 (cos' = 0 at 0; the Gaussian envelope's is 0
    at 0; the exponential envelope's is taken as 0, autodiff._SqrtZeroGrad), by alpha it is 1, by omega and gamma 0."""
    rng = np.random.default_rng(11 + d)
    P = _Pair(lib, 5, d, family, rng, same=True)
    v, g = P.grad()
    assert abs(v - P.alpha.sum()) <= 1e-14 * P.alpha.sum()
    for name, arr in g.items():
        assert np.all(np.isfinite(arr)), name
    for name in ("x", "y", "omega", "gamma"):
        assert np.all(g[name] == 0.0), name
    assert np.all(g["alpha"] == 1.0)
