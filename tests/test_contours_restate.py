"""CPU: the two restatements of cv.findContours(RETR_TREE) filtered to parent -1 (tests/contours_restate.py) against each other
and against hand cases; the arguments that the contour calls refuse before they touch a device."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contours_restate as R  # noqa: E402

METHODS = (R.CHAIN_APPROX_NONE, R.CHAIN_APPROX_SIMPLE)


def lists(contours):
    return [[tuple(p) for p in c.tolist()] for c in contours]


@pytest.mark.parametrize('method', METHODS)
def test_the_two_restatements_agree(method):
    """400 seeded masks up to 39 x 39, densities 0.05 .. 0.95, every fourth dilated into blobs"""
    rng = default_rng(20240607 + method)
    kept = 0
    for k in range(400):
        mask = R.random_mask(rng, blobs=k % 4 == 3)
        got = R.contours_scan(mask, method)
        R.same_contours(got, R.contours_label(mask, method))
        kept += len(got)
    assert kept > 400          # the sweep is no sweep of empty planes


def test_hand_cases():
    rect = np.zeros((6, 9), np.uint8)
    rect[1:4, 2:7] = 1
    row = np.zeros((3, 5), np.uint8)
    row[1, 1:4] = 1
    ring = np.ones((7, 7), np.uint8)
    ring[1:6, 1:6] = 0
    ring[3, 3] = 1
    diagonal = np.zeros((3, 4), np.uint8)
    diagonal[0, 0] = diagonal[1, 1] = diagonal[2, 2] = diagonal[0, 3] = 1
    for contours in (R.contours_scan, R.contours_label):
        assert lists(contours(rect, R.CHAIN_APPROX_SIMPLE)) == [[(2, 1), (2, 3), (6, 3), (6, 1)]]
        (points,) = contours(rect, R.CHAIN_APPROX_NONE)
        assert len(points) == 12 and tuple(points[0]) == (2, 1)
        assert lists(contours(row, R.CHAIN_APPROX_SIMPLE)) == [[(1, 1), (3, 1)]]
        assert lists(contours(ring, R.CHAIN_APPROX_SIMPLE)) == [[(0, 0), (0, 6), (6, 6), (6, 0)]]
        assert lists(contours(diagonal, R.CHAIN_APPROX_SIMPLE)) == [[(0, 0), (2, 2)], [(3, 0)]]
        assert contours(np.zeros((4, 5), np.uint8)) == []
        # values above 1 are foreground like 1
        assert lists(contours(rect * 255, R.CHAIN_APPROX_SIMPLE)) == lists(contours(rect, R.CHAIN_APPROX_SIMPLE))


def test_emitted_points_are_bounded_by_the_foreground():
    """CHAIN_APPROX_NONE: a border enters a pixel from at most four sides, so at most 4 points a foreground pixel"""
    rng = default_rng(7)
    for k in range(100):
        mask = R.random_mask(rng, 60, 60, blobs=k % 2 == 1)
        total = sum(len(c) for c in R.contours_scan(mask, R.CHAIN_APPROX_NONE))
        assert total <= 4 * int((mask > 0).sum())
        for simple, full in zip(R.contours_scan(mask, R.CHAIN_APPROX_SIMPLE), R.contours_scan(mask, R.CHAIN_APPROX_NONE)):
            assert len(simple) <= len(full) and tuple(simple[0]) == tuple(full[0])


def test_unknown_method_in_the_restatement():
    with pytest.raises(ValueError):
        R.contours_scan(np.ones((2, 2), np.uint8), 3)
    with pytest.raises(ValueError):
        R.contours_label(np.ones((2, 2), np.uint8), 4)


def test_refusals_come_before_any_device_call(monkeypatch):
    """keep_internal=True and an unknown method code raise on a host-backed mask without a context being made"""
    from vkit_amd import _native as N
    from vkit_amd.element import Mask
    from vkit_amd.element.mask import masks_to_disconnected_polygons

    def no_device(*args, **kwargs):
        raise AssertionError('a device call')

    monkeypatch.setattr(N, 'default_ctx', no_device)
    monkeypatch.setattr(N, 'lib', no_device)
    mask = Mask(mat=np.ones((3, 4), np.uint8))
    with pytest.raises(NotImplementedError):
        mask.to_disconnected_polygons(keep_internal=True)
    with pytest.raises(NotImplementedError):
        masks_to_disconnected_polygons([mask], keep_internal=True)
    for method in (0, 3, 4, -1):
        with pytest.raises(ValueError):
            mask.to_disconnected_polygons(cv_find_contours_method=method)
        with pytest.raises(ValueError):
            mask.to_external_polygon(cv_find_contours_method=method)
        with pytest.raises(ValueError):
            mask.to_disconnected_polygon_mask_pairs(cv_find_contours_method=method)
        with pytest.raises(ValueError):
            N.mask_contours([], method)
    assert masks_to_disconnected_polygons([]) == [] and N.mask_contours([]) == []


def test_polygon_area_is_the_shoelace_sum():
    from vkit_amd.element import Polygon
    assert Polygon.from_np_array(np.array([(2, 1), (2, 3), (6, 3), (6, 1)], np.int32)).area == 8.0
    assert Polygon.from_np_array(np.array([(0, 0), (4, 0), (0, 3)], np.int32)).area == 6.0
