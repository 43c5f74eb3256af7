"""fmri_hip.ops.zoom_geometry (the host half of zoom_f64: output shape and coordinate ratio per axis) against the shapes
scipy.ndimage.zoom itself returns - including Python's round-half-to-even (5 * 0.5 -> 2) and axes of length 1 on either side."""
import numpy as np
import pytest
from scipy import ndimage

FACTORS = [(1.6, 0.7, 2.0), (0.5, 1.3, 1.0), (1 / 0.7, 1 / 0.7, 1 / 1.3)]
CASES = [((7, 9, 5), f) for f in FACTORS] + [((33, 40, 6), f) for f in FACTORS] + [
    ((1, 4, 3), (3.0, 0.5, 1.0)),          # an input axis of length 1
    ((4, 5, 3), (0.25, 1, 1)),             # an output axis of length 1
    ((5, 4, 3), (0.5, 1, 1)),              # 2.5 -> 2
    ((4, 3, 2), (47.0, 1, 1)),             # 4 -> 188
]


@pytest.mark.parametrize("shape,factors", CASES)
def test_zoom_geometry_equals_scipy(shape, factors):
    from fmri_hip.ops import zoom_geometry
    out_shape, ratios = zoom_geometry(shape, factors)
    want = ndimage.zoom(np.zeros(shape, dtype=np.uint8), factors, order=0).shape
    assert out_shape == want
    for n, m, r in zip(shape, out_shape, ratios):
        assert isinstance(r, float)
        assert r == ((n - 1) / (m - 1) if m > 1 else 1.0)


def test_zoom_geometry_rounds_halves_to_even_and_broadcasts_a_scalar():
    from fmri_hip.ops import zoom_geometry
    assert zoom_geometry((5, 4, 3), (0.5, 1, 1))[0] == (2, 4, 3)
    assert zoom_geometry((7, 3, 3), (0.5, 1, 1))[0] == (4, 3, 3)           # 3.5 -> 4
    assert zoom_geometry((6, 6, 6), 0.5) == ((3, 3, 3), (2.5, 2.5, 2.5))
