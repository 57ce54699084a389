"""Which low-rank SignatureSpectral feature maps take the spectral cross op and the kernels behind the cross matrix (autodiff._lr_spectral_wide):
33 .. 4096 columns within the limits of those kernels; nothing at 32 columns and below, where the fused spectral ops and _lr_route decide as they
did -- and _lr_route itself still never answers "kx" for this family.  No GPU."""
import pytest

from gpsig_amd import autodiff

LT = lambda M: M * (M + 1) // 2


@pytest.mark.parametrize("d", [1, 3, 16, 32])
def test_narrow_state_spaces_keep_their_ops(d):
    for cc in (1, 16, 50, 64, 65):
        for r in (1, 16, 50, 64, 200):
            for M in (1, 2, 4, 8, 10):
                assert not autodiff._lr_spectral_wide(cc, r, d, M)
                assert not autodiff._lr_spectral_wide(cc, r, d, M, tens=(LT(M), 2))
                assert not autodiff._lr_spectral_wide(cc, r, d, M, tens=(LT(M), 1))


@pytest.mark.parametrize("d", [33, 63, 964, 4096])
def test_wide_state_spaces_take_the_cross_op(d):
    assert autodiff._lr_spectral_wide(50, 50, d, 4)
    assert autodiff._lr_spectral_wide(50, 50, d, 4, tens=(10, 2))


@pytest.mark.parametrize("d", [33, 63, 964, 4096])
def test_beyond_the_limits_of_the_ops_behind_it(d):
    assert not autodiff._lr_spectral_wide(65, 50, d, 4)
    assert not autodiff._lr_spectral_wide(65, 50, d, 4, tens=(10, 2))
    assert not autodiff._lr_spectral_wide(50, 50, d, 10)
    assert not autodiff._lr_spectral_wide(50, 50, d, 10, tens=(LT(10), 2))
    assert not autodiff._lr_spectral_wide(50, 50, d, 4, tens=(9, 2))


def test_beyond_the_cross_op():
    assert not autodiff._lr_spectral_wide(50, 50, 4097, 4)
    assert not autodiff._lr_spectral_wide(50, 50, 4097, 4, tens=(10, 2))


@pytest.mark.parametrize("d", [3, 32, 33, 63, 964, 4096])
def test_the_route_table_never_answers_kx_for_this_family(d):
    for cc, M in ((50, 4), (65, 4), (50, 10)):
        for L, dense in ((40, True), (40, False), (500, True)):
            assert autodiff._lr_route(cc, 50, d, M, L, True, dense) != "kx"
        for tens in ((10, 2), (9, 2), (LT(M), 1)):
            assert autodiff._lr_route(cc, 50, d, M, 0, True, True, tens=tens) != "kx"
