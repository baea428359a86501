"""CPU: tests/radar_dx_reference.py -- the hand-written float64 adjoint of the VirtualRadar signal stage with respect to the
skeleton -- against float64 autograd of oracle.radar.signal_torch at generic points, and its zero-subgradient conventions at the
degenerate points where autograd is NaN (an absent body, a joint at the radar position, a zero-length edge, an unused joint)."""
import numpy as np
import pytest

import radar_dx_reference as X
from oracle import radar as R

LOC = (0.5, -1.0, 2.0)
HUB_EDGES = [(0, 1), (1, 2), (1, 3), (1, 4), (4, 5)]      # 7 joints: joint 1 is a hub of four edges, joint 6 is in no edge


@pytest.mark.parametrize("lam", [10.0, 0.1, 5e-4])
def test_equals_float64_autograd_on_the_ntu_graph(lam):
    x = X.synthetic_clip(2, 9)
    ur, ui = X.cotangent(2, 9)
    want = X.autograd_dx(x, LOC, lam, ur, ui, R.EDGES)
    assert np.isfinite(want).all()
    got = X.signal_dx(x, LOC, lam, ur, ui, R.EDGES)
    assert got.shape == x.shape and got.dtype == np.float64
    assert X.rel_err(got, want) < 1e-10


@pytest.mark.parametrize("lam", [10.0, 0.1, 5e-4])
def test_equals_float64_autograd_on_a_custom_graph_with_a_hub_and_an_unused_joint(lam):
    x = X.synthetic_clip(2, 9, V=7, M=2, seed=3)
    ur, ui = X.cotangent(2, 9, seed=4)
    want = X.autograd_dx(x, LOC, lam, ur, ui, HUB_EDGES)
    assert np.isfinite(want).all()
    got = X.signal_dx(x, LOC, lam, ur, ui, HUB_EDGES)
    assert X.rel_err(got, want) < 1e-10
    assert (got[:, :, :, 6] == 0).all() and (want[:, :, :, 6] == 0).all()
    assert np.abs(got[:, :, :, 1]).min() > 0


def test_an_absent_body_gets_exactly_zero_and_leaves_the_other_body_alone():
    """the documented deviation: autograd is NaN in every coordinate of the absent body (sqrt'(0) * 0 in the RCS)"""
    x = X.synthetic_clip(2, 9)
    x[:, :, :, :, 1] = 0
    ur, ui = X.cotangent(2, 9)
    got = X.signal_dx(x, LOC, 0.1, ur, ui, R.EDGES)
    assert np.isfinite(got).all()
    assert (got[..., 1] == 0).all()
    one = X.signal_dx(x[..., :1], LOC, 0.1, ur, ui, R.EDGES)
    assert np.array_equal(got[..., :1], one) and np.abs(one).max() > 0
    assert X.rel_err(one, X.autograd_dx(x[..., :1], LOC, 0.1, ur, ui, R.EDGES)) < 1e-10
    auto = X.autograd_dx(x, LOC, 0.1, ur, ui, R.EDGES)
    assert np.isnan(auto[..., 1]).all()


def test_a_joint_at_the_radar_and_a_zero_length_edge_give_finite_gradients():
    x = X.synthetic_clip(2, 9)
    x[0, :, 2, 20, 0] = np.asarray(LOC, dtype=np.float32)       # the spine joint (source of three edges) at the radar position
    x[1, :, 4, 5, 1] = x[1, :, 4, 4, 1]                         # edge (4, 5) of body 1 has length 0 in frame 4
    ur, ui = X.cotangent(2, 9)
    for lam in (10.0, 5e-4):
        got = X.signal_dx(x, LOC, lam, ur, ui, R.EDGES)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
    # the untouched frames are what autograd gives
    lam = 0.1
    got, auto = X.signal_dx(x, LOC, lam, ur, ui, R.EDGES), X.autograd_dx(x, LOC, lam, ur, ui, R.EDGES)
    keep = np.ones(9, dtype=bool)
    keep[[2, 4]] = False
    assert X.rel_err(got[:, :, keep], auto[:, :, keep]) < 1e-10


def test_the_band_rule():
    assert X.within_band(1.9e-5, 0.0) and not X.within_band(2.1e-5, 0.0)
    assert X.within_band(2.9e-4, 1e-4) and not X.within_band(3.1e-4, 1e-4)
    assert X.within_band(7e-4, 1e-4, factor=8)
