"""kurosiwo_amd.dataset.slope_riserun (the host side of --slope, dataset/Dataset.py:747-761) pinned by hand, and the C-ABI entry point
that computes the same on the device (ksmi_dem_slope: exported, bound, argument checks that launch nothing).  No GPU."""
import math

import numpy as np

from kurosiwo_amd import _lib
from kurosiwo_amd.dataset import slope_riserun

F32_SENTINEL = float(np.float32(3.4e38))        # what a float32 DEM tile holds where the file says 3.4e38


def _ramp():
    y, x = np.mgrid[0:3, 0:3]
    return (2 * x + 3 * y).astype(np.float32)


def test_ramp_every_cell_by_hand():
    """z[y, x] = 2x + 3y on 3 x 3.  Edge rule: a neighbour outside the grid takes the centre's value, so relative to the centre it
    contributes 0 and an in-grid neighbour (dy, dx) contributes 2 dx + 3 dy.  The pairs (8 dzdx, 8 dzdy) below are those sums written
    out per cell, e.g. the corner (0, 0) sees (0,1) = 2, (1,0) = 3, (1,1) = 5: 8 dzdx = 2*2 + 5 = 9, 8 dzdy = 2*3 + 5 = 11; the
    centre sees all eight: 8 dzdx = 4 + 8 + 4 = 16, 8 dzdy = 6 + 12 + 6 = 24, slope sqrt(2^2 + 3^2) = sqrt(13).  The one-sided
    differences of an edge cell weigh half of the two-sided ones of the interior (the missing side adds nothing)."""
    eighths = [[(9, 11), (12, 12), (3, 7)],
               [(8, 18), (16, 24), (8, 18)],
               [(3, 7), (12, 12), (9, 11)]]
    want = np.array([[math.sqrt((p / 8.0) ** 2 + (q / 8.0) ** 2) for p, q in row] for row in eighths]).astype(np.float32)
    got = slope_riserun(_ramp())
    assert got.dtype == np.float32 and got.shape == (3, 3)
    assert np.array_equal(got, want)
    assert got[1, 1] == np.float32(math.sqrt(13.0))


def test_single_cell_is_flat():
    assert np.array_equal(slope_riserun(np.array([[7.5]], dtype=np.float32)), np.zeros((1, 1), dtype=np.float32))


def test_nan_neighbour_counts_as_outside_the_grid():
    """the centre of a 3 x 3 whose right column is NaN == the right-edge cell of the 3 x 2 grid without that column"""
    z = _ramp()
    cut = z[:, :2].copy()
    z[:, 2] = np.nan
    got = slope_riserun(z)
    assert np.array_equal(got[:, 1], slope_riserun(cut)[:, 1]) and np.array_equal(got[:, 0], slope_riserun(cut)[:, 0])
    # by hand for the middle row: in-grid neighbours (-1,-1) = -5, (-1,0) = -3, (0,-1) = -2, (1,-1) = 1, (1,0) = 3
    assert got[1, 1] == np.float32(math.sqrt(((0 - (-5 - 4 + 1)) / 8.0) ** 2 + (((1 + 6) - (-5 - 6)) / 8.0) ** 2))


def test_nan_centre_gives_nan():
    """a NaN centre hands its NaN to every neighbour slot it fills in (outside the grid or NaN itself), and the sums carry it.  Horn's
    differences never read the centre itself, so the one NaN cell that does NOT give NaN is an interior one whose eight neighbours are
    all valid: it gets their slope (here the ramp's sqrt(13)); DEM tiles reach this function gap-filled, without NaN."""
    assert np.isnan(slope_riserun(np.array([[np.nan]], dtype=np.float32))[0, 0])
    z = _ramp()
    z[0, 0] = np.nan
    z[2, 1] = np.nan
    got = slope_riserun(z)
    assert np.isnan(got[0, 0]) and np.isnan(got[2, 1])
    z = np.full((3, 3), np.nan, dtype=np.float32)
    assert np.isnan(slope_riserun(z)).all()
    z = np.pad(_ramp(), 1, mode="edge")
    z[2, 2] = np.nan
    z[2, 3] = np.nan
    assert np.isnan(slope_riserun(z)[2, 2]) and np.isnan(slope_riserun(z)[2, 3])           # an interior NaN next to a NaN
    z = _ramp()
    z[1, 1] = np.nan
    assert slope_riserun(z)[1, 1] == np.float32(math.sqrt(13.0))


def test_sentinel_is_compared_as_a_double():
    """float(np.float32(3.4e38)) is the value the widened cells hold: recognised.  3.4e38 itself is no float32: it equals no cell, the
    sentinel cells stay ordinary (huge) heights."""
    z = np.pad(_ramp(), 1, mode="edge")                    # 5 x 5
    z[1, 3] = np.float32(3.4e38)
    z[4, 0] = np.float32(3.4e38)
    hole = z.copy()
    hole[1, 3] = hole[4, 0] = np.nan
    with np.errstate(all="ignore"):
        seen, unseen, plain = slope_riserun(z, F32_SENTINEL), slope_riserun(z, 3.4e38), slope_riserun(z)
        as_nan = slope_riserun(hole)
    assert seen[1, 3] == np.float32(3.4e38) and seen[4, 0] == np.float32(3.4e38)
    keep = np.ones_like(z, dtype=bool)
    keep[1, 3] = keep[4, 0] = False
    assert np.array_equal(seen[keep], as_nan[keep]) and np.isfinite(seen).all() and seen[keep].max() < 10.0
    assert np.array_equal(unseen, plain)
    assert unseen[1, 3] != np.float32(3.4e38) and unseen[1, 2] > 1e36 and unseen[3, 0] > 1e36
    assert np.array_equal(slope_riserun(z, float("nan")), plain)


def test_library_exports_dem_slope():
    lib = _lib.load()
    assert hasattr(lib, "ksmi_dem_slope") and "ksmi_dem_slope" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["ksmi_dem_slope"]
    assert res is _lib.C.c_int and len(args) == 10 and args[5] is _lib.C.c_double and args[-1] is _lib.C.c_void_p


def test_argument_errors_launch_nothing():
    """refused before any HIP call, so this runs without a device; the pointers are never dereferenced"""
    fn = _lib.load().ksmi_dem_slope
    nan = float("nan")
    a, b = 0x10000, 0x10000 + 2 * 3 * 5 * 4
    assert fn(a, b, 0, 3, 5, nan, 0.0, 1.0, 0, None) == 0
    assert fn(None, None, 0, 3, 5, nan, 0.0, 1.0, 0, None) == 0
    for bad in ((a, b, 2, 0, 5), (a, b, 2, 3, 0), (a, b, -1, 3, 5), (None, b, 2, 3, 5), (a, None, 2, 3, 5), (a, a, 2, 3, 5), (a, b - 4, 2, 3, 5)):
        assert fn(*bad, nan, 0.0, 1.0, 0, None) < 0, bad
        assert b"dem_slope" in _lib.load().ksmi_last_error()
