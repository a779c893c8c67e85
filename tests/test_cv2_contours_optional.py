"""Pins the contour restatement (tests/contours_restate.py) against a real OpenCV -- only where one is installed.

The build image has no cv2, so these tests are skipped there and the contours stay "unpinned at the cv2 boundary" (DESIGN.md
section 2), the order of the contours included.  Where cv2 imports: cv.findContours(mask * 255, RETR_TREE, method) filtered to
hierarchy parent -1, first as a set of contours (each exact, its start point included), then by order."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

cv = pytest.importorskip('cv2')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contours_restate as R  # noqa: E402


def cv_contours(mask, method):
    contours, hierarchy = cv.findContours((mask > 0).astype(np.uint8) * 255, cv.RETR_TREE, method)
    if not contours:
        return []
    return [np.squeeze(c, axis=1).astype(np.int32) for c, h in zip(contours, hierarchy[0]) if h[3] < 0]


def masks():
    rng = default_rng(11)
    for k in range(300):
        yield R.random_mask(rng, 64, 64, blobs=k % 3 == 2)


@pytest.mark.parametrize('method', [cv.CHAIN_APPROX_NONE, cv.CHAIN_APPROX_SIMPLE])
def test_the_same_set_of_contours(method):
    assert (cv.CHAIN_APPROX_NONE, cv.CHAIN_APPROX_SIMPLE) == (R.CHAIN_APPROX_NONE, R.CHAIN_APPROX_SIMPLE)
    for mask in masks():
        ours = sorted(tuple(map(tuple, c.tolist())) for c in R.contours_scan(mask, method))
        theirs = sorted(tuple(map(tuple, c.tolist())) for c in cv_contours(mask, method))
        assert ours == theirs


@pytest.mark.parametrize('method', [cv.CHAIN_APPROX_NONE, cv.CHAIN_APPROX_SIMPLE])
def test_the_same_order(method):
    for mask in masks():
        R.same_contours(R.contours_scan(mask, method), cv_contours(mask, method))
