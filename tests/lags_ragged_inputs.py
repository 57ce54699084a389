"""What the tests of ragged batches with lags share: the check each test module runs on its own (lengths, lags) before anything else.

The lag interpolant (gpsig/lags.py:20-33) jumps where a query crosses a bracket's flip point t_i - 1e-6, and the gradient of the lags jumps
where a query meets the clamp at 0: two correct implementations may land on either side of such a point.  The tests therefore use lengths and
lags whose queries keep a margin of 1e-9 from both -- pure arithmetic on the host."""
import numpy as np

JITTER = 1e-6
MARGIN = 1e-9
LAGS = (0.137, 0.41, 0.93, 0.004)        # two odd values, one that clamps most queries, one shorter than a step of every axis used


def check_inputs(lengths, lags):
    """Asserts that no query of any (sequence length, observation, lag) lies within MARGIN of a flip point or of the clamp.  Returns the
    smallest distance found (inf where nothing was compared)."""
    closest = np.inf
    for length in sorted(set(int(l) for l in lengths)):
        if length < 2:
            continue                                    # one point: no axis, no query
        axis = np.arange(length, dtype=np.float64) / (length - 1)
        for lag in lags:
            raw = axis - float(lag)
            clamp = np.abs(raw).min()
            assert clamp > MARGIN, ("a query at the clamp", length, lag, clamp)
            tq = np.maximum(raw, 0.0)
            flip = np.abs((axis[:, None] - JITTER) - tq[None, :]).min()
            assert flip > MARGIN, ("a query at a flip point", length, lag, flip)
            closest = min(closest, clamp, flip)
    return closest
