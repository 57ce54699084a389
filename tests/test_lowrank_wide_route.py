"""The route table of low-rank training (autodiff._lr_route): which ops compute a feature map of (components, rank, columns, levels).  "fused"
must be exactly where the ops that take the points were used before the cross matrix became an op of its own -- computed here from _lr_limits
itself --, "kx" where they were out only because of the number of columns, "torch" everything else.  No GPU."""
import pytest

from gpsig_amd import autodiff

L = 100


def _before(cc, r, d, M, spectral=False, dense=True, L=L):
    """what _LowRankScope._seq_hip decided before _lr_route existed: the HIP ops or torch"""
    sizes_ok, tile_fits = autodiff._lr_limits(cc, r, d, M)
    whole = 8 * ((L + 63) // 64 * 64 + 1) * 4 * max(cc, r, d, 16) <= 156 * 1024
    return sizes_ok and (tile_fits or (spectral and dense and whole))


@pytest.mark.parametrize("cc,r,d,M", [(50, 50, 3, 4), (50, 50, 75, 4), (64, 64, 64, 4)])
def test_served_shapes_keep_their_route(cc, r, d, M):
    want = "fused" if _before(cc, r, d, M) else "kx"
    assert autodiff._lr_route(cc, r, d, M, L, False, True) == want
    assert autodiff._lr_route(cc, r, d, M, L, False, False) == want
    if (cc, d) in ((50, 3), (64, 64)):
        assert want == "fused"


@pytest.mark.parametrize("cc,r,d,M", [(50, 50, 126, 4), (64, 64, 65, 4), (16, 16, 300, 4), (50, 50, 1928, 4)])
def test_wide_state_spaces_take_the_cross_op(cc, r, d, M):
    assert not _before(cc, r, d, M)
    for dense in (True, False):
        assert autodiff._lr_route(cc, r, d, M, L, False, dense) == "kx"


@pytest.mark.parametrize("d", [3, 24, 65, 126, 1928])
def test_everything_else_is_as_before(d):
    # more than 64 components and more than 8 levels: torch at every width
    assert autodiff._lr_route(65, 65, d, 4, L, False, True) == "torch"
    assert autodiff._lr_route(50, 50, d, 10, L, False, True) == "torch"
    # SignatureSpectral: never "kx"
    for cc, Ls, dense in ((16, 40, True), (16, 40, False), (50, 100, True), (64, 500, True)):
        got = autodiff._lr_route(cc, cc, d, 4, Ls, True, dense)
        assert got == ("fused" if _before(cc, cc, d, 4, True, dense, Ls) else "torch")


def test_tensor_route():
    lt = lambda M: M * (M + 1) // 2
    assert autodiff._lr_route(50, 50, 3, 4, 0, False, True, tens=(lt(4), 2)) == "fused"
    assert autodiff._lr_route(50, 50, 126, 4, 0, False, True, tens=(lt(4), 2)) == "kx"
    assert autodiff._lr_route(16, 16, 300, 2, 0, False, True, tens=(lt(2), 1)) == "kx"
    assert autodiff._lr_route(50, 50, 126, 4, 0, True, True, tens=(lt(4), 2)) == "torch"
    assert autodiff._lr_route(65, 65, 126, 4, 0, False, True, tens=(lt(4), 2)) == "torch"
    assert autodiff._lr_route(50, 50, 126, 4, 0, False, True, tens=(lt(4) - 1, 2)) == "torch"
