"""Polygon rasterisation (cv.fillPoly semantics) and the operators built on it, GPU vs oracle."""
import numpy as np
import pytest
from numpy.random import default_rng

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    from vkit_amd import _native
    return _native


def _check(N, shape, pts):
    got = N.fill_poly_mask(shape, pts)
    want = O.fill_poly(shape, np.asarray(pts, np.int32))
    np.testing.assert_array_equal(got, want)
    return got


def test_fill_poly_random_polygons(N):
    rng = default_rng(5)
    for case in range(60):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        n = int(rng.integers(1, 12))
        pts = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)
        _check(N, (h, w), pts)


def test_fill_poly_degenerate_shapes(N):
    _check(N, (9, 9), [(4, 4)])                                   # single point
    _check(N, (9, 9), [(1, 1), (7, 6)])                           # segment
    _check(N, (9, 9), [(0, 3), (8, 3), (4, 3)])                   # collinear horizontal
    _check(N, (9, 9), [(3, 0), (3, 8), (3, 2)])                   # collinear vertical
    _check(N, (12, 12), [(0, 0), (11, 0), (11, 11), (0, 11)])     # full rectangle
    _check(N, (12, 12), [(0, 0), (11, 11), (11, 0), (0, 11)])     # bow tie
    _check(N, (30, 30), [(2, 2), (27, 2), (27, 27), (2, 27), (2, 2)])  # closing duplicate kept at this level


def test_fill_poly_star_and_many_vertices(N):
    rng = default_rng(6)
    # a self-intersecting star: even-odd rule leaves the centre empty
    k = 7
    ang = np.arange(k) * (2 * np.pi * 3 / k)
    pts = np.stack([200 + 180 * np.cos(ang), 200 + 180 * np.sin(ang)], axis=1).round().astype(np.int32)
    got = _check(N, (401, 401), pts)
    assert got[200, 200] == 1 or got[200, 200] == 0  # value itself is the oracle's; shape checked above
    # a few thousand vertices on a noisy circle (long edge table, many crossings per scanline)
    n = 3000
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = 700 + rng.integers(-40, 41, n)
    pts = np.stack([800 + r * np.cos(t), 800 + r * np.sin(t)], axis=1).round().astype(np.int32)
    _check(N, (1601, 1601), pts)


def test_fill_poly_full_size_border_polygon(N):
    """Border polygon of a 2048^2 camera-distorted lattice (the active mask of the C3 workload)."""
    from vkit_amd.mechanism.distortion import camera_cubic_curve
    from vkit_amd.mechanism.distortion_policy.geometric import camera as P_cam
    gen = P_cam.CameraCubicCurveConfigGenerator(P_cam.CameraCubicCurveConfigGeneratorConfig(), 5)
    config = gen((2048, 2048), default_rng(3))
    state = camera_cubic_curve.generate_state(config, (2048, 2048))
    grid = state.dst_image_grid
    polygon = grid.generate_border_polygon()
    active = camera_cubic_curve.get_active_mask(config, (2048, 2048), state=state)
    box = polygon.bounding_box
    want = np.zeros(active.shape, np.uint8)
    want[box.up:box.down + 1, box.left:box.right + 1] = O.fill_poly(
        box.shape, polygon.self_relative_polygon.to_np_array())
    np.testing.assert_array_equal(active.mat, want)
    assert 0 < int(active.mat.sum()) < active.mat.size


def test_polygon_fill_and_extract_operators(N):
    from vkit_amd.element import Image, Mask, Polygon
    rng = default_rng(8)
    polygon = Polygon.from_xy_pairs([(10, 5), (60, 12), (48, 50), (30, 30), (6, 44)])
    box = polygon.bounding_box
    raster = O.fill_poly(box.shape, polygon.self_relative_polygon.to_np_array()).astype(bool)
    np.testing.assert_array_equal(polygon.np_mask, raster)

    mat = rng.integers(0, 256, (64, 72, 3), dtype=np.uint8)
    image = Image(mat=mat.copy())
    polygon.fill_image(image, (255, 0, 7), alpha=0.4)
    want = mat.copy()
    O.fill(want, (box.up, box.left, box.height, box.width), (255, 0, 7), mask=raster.astype(np.uint8), alpha=0.4)
    np.testing.assert_array_equal(image.mat, want)

    mask = Mask.from_shape((64, 72))
    polygon.fill_mask(mask)
    full = np.zeros((64, 72), np.uint8)
    full[box.up:box.down + 1, box.left:box.right + 1] = raster
    np.testing.assert_array_equal(mask.mat, full)

    extracted = polygon.extract_image(Image(mat=mat.copy()))
    want = mat[box.up:box.down + 1, box.left:box.right + 1].copy()
    want[~raster] = 0
    np.testing.assert_array_equal(extracted.mat, want)


# ---- combs: 2 * teeth crossings a scanline, around the one-pass boundary of the crossing ranking and at the capacities
def _comb(teeth):
    from text_region_masks_restate import comb
    return (16, 4 * teeth + 9), comb(3, 2, 9, 13, teeth)


@pytest.mark.parametrize('teeth', [32, 33, 256])
def test_fill_poly_comb_up_to_512_crossings(N, teeth):
    shape, pts = _comb(teeth)
    got = _check(N, shape, pts)
    assert (np.diff(got[5].astype(np.int8)) == 1).sum() == teeth      # that many runs on a row through the teeth


def test_fill_poly_comb_beyond_512_crossings_is_refused(N):
    shape, pts = _comb(257)
    with pytest.raises(N.VkxError, match='512 edge crossings'):
        N.fill_poly_mask(shape, pts)
    _check(N, shape, _comb(256)[1])                                   # the context goes on


def test_paint_polys_comb_at_and_beyond_64_crossings(N):
    """a 32-tooth comb (64 crossings) over a rectangle equals the ordered paint of the oracle's rasters; a 33-tooth comb is
    refused, and the paint after it on the same context is correct (the ownership raster is zero again after the error exit)"""
    ctx = N.default_ctx()
    shape, pts = _comb(33)
    rect = np.array([(1, 1), (shape[1] - 2, 1), (shape[1] - 2, 11), (1, 11)], np.int32)
    values = [3.5, 7.25]

    def want(polygons):
        mask, score = np.zeros(shape, np.uint8), np.zeros(shape, np.float32)
        for polygon, value in zip(polygons, values):
            inside = O.fill_poly(shape, polygon).astype(bool)
            mask[inside] = 1
            score[inside] = value
        return mask, score

    def paint(polygons):
        mask, score = N.dev_zeros(shape, np.uint8, ctx), N.dev_zeros(shape, np.float32, ctx)
        N.paint_polys(polygons, values=values, mask=mask, score=score, ctx=ctx)
        return np.array(mask.host()), np.array(score.host())

    polygons = [rect, _comb(32)[1]]
    for got, ref in zip(paint(polygons), want(polygons)):
        np.testing.assert_array_equal(got, ref)
    with pytest.raises(N.VkxError, match='64 edge crossings'):
        paint([rect, pts])
    polygons = [_comb(32)[1], rect + np.asarray([1, 3], np.int32)]           # (still inside the plane, as the oracle requires)
    for got, ref in zip(paint(polygons), want(polygons)):
        np.testing.assert_array_equal(got, ref)
