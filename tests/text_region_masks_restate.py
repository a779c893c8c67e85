"""numpy-plus-oracle restatement of TextRegionFlattener.get_bounding_extended_text_region_masks (reference: pipeline/
text_detection/page_text_region.py:477-558) for the tests of csrc/region_masks.hip, and the synthetic pages those tests and
tests/golden/make_text_region_masks_golden.py share.

The reference's sequence of fills, inversions and count planes, pixel by pixel over the region's box BB (the union of the
boxes of the dilated polygon D and the bounding rectangular polygon R), with T the union of the rasters of ALL original polygons
and o, d, r the rasters of the region's O, D and R:

    out = (d and not (r and T and not o)) or (r and not T)

Every raster is the polygon's own cv.fillPoly mask over its bounding box (the oracle's fill_poly), placed at that box.
"""
import json
import os

import numpy as np

import oracle as O

ANGLES = (0, 1, 45, 89, 90, 91, 135, 179)
PAGES = ((96, 128), (61, 203))
COUNTS = (1, 3, 70)


def bounding_box(points):
    """(up, down, left, right) of int (n, 2) (x, y) points"""
    points = np.asarray(points)
    return int(points[:, 1].min()), int(points[:, 1].max()), int(points[:, 0].min()), int(points[:, 0].max())


def union_box(a, b):
    return min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3])


def np_mask(points):
    """PolygonInternals.np_mask: the raster of the self-relative polygon over its bounding box, and that box"""
    points = np.asarray(points, np.int32).reshape(-1, 2)
    up, down, left, right = box = bounding_box(points)
    return O.fill_poly((down - up + 1, right - left + 1), np.ascontiguousarray(points - (left, up), dtype=np.int32)) > 0, box


def placed(points, target):
    """the polygon's raster in the frame of the box `target`; the polygon's box must lie inside it (element/box.py:227-228)"""
    raster, (up, down, left, right) = np_mask(points)
    t_up, t_down, t_left, t_right = target
    if not (t_up <= up and down <= t_down and t_left <= left and right <= t_right):
        raise AssertionError('a filling polygon whose box leaves the target box')
    plane = np.zeros((t_down - t_up + 1, t_right - t_left + 1), np.bool_)
    plane[up - t_up:down - t_up + 1, left - t_left:right - t_left + 1] = raster
    return plane


def text_mask(shape, originals):
    page = (0, shape[0] - 1, 0, shape[1] - 1)
    T = np.zeros(shape, np.bool_)
    for points in originals:
        T |= placed(points, page)
    return T


def extended_masks(shape, originals, dilated, rectangles, T=None):
    """[(uint8 mask, (up, down, left, right))] a region; `rectangles` already patched for the non-typical regions"""
    if T is None:
        T = text_mask(shape, originals)
    out = []
    for o_pts, d_pts, r_pts in zip(originals, dilated, rectangles):
        box = union_box(bounding_box(d_pts), bounding_box(r_pts))
        o, d, r = placed(o_pts, box), placed(d_pts, box), placed(r_pts, box)
        t = T[box[0]:box[1] + 1, box[2]:box[3] + 1]
        out.append((((d & ~(r & t & ~o)) | (r & ~t)).astype(np.uint8), box))
    return out


# ---- the synthetic pages -----------------------------------------------------------------------------------------------
def clip(points, shape):
    points = np.rint(np.asarray(points, np.float64)).astype(np.int32).reshape(-1, 2)
    points[:, 0] = np.clip(points[:, 0], 0, shape[1] - 1)
    points[:, 1] = np.clip(points[:, 1], 0, shape[0] - 1)
    return points


def comb(x0, y0, ym, y1, teeth):
    """a concave comb of 4 * teeth vertices: teeth of 2 px every 4 px from y0 down to a bar [ym, y1]; 2 * teeth crossings a
    scanline between y0 and ym"""
    pts = [(x0, y1)]
    for i in range(teeth):
        xa = x0 + 4 * i
        pts += [(xa, y0), (xa + 2, y0)]
        if i < teeth - 1:
            pts += [(xa + 2, ym), (xa + 4, ym)]
    pts.append((x0 + 4 * (teeth - 1) + 2, y1))
    assert len(pts) == 4 * teeth
    return np.array(pts, np.int32)


def rotated_rectangle(cx, cy, a, b, theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([(cx + u * a * c - v * b * s, cy + u * a * s + v * b * c) for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))])


def box_polygon(box, pad, shape):
    up, down, left, right = box
    return clip([(left - pad, up - pad), (right + pad, up - pad), (right + pad, down + pad), (left - pad, down + pad)], shape)


def random_region(rng, shape):
    """a jittered rotated quadrilateral O; D is O or O scaled by 1.3 about its centre; R is D's box padded, or a thin rotated
    rectangle that does NOT contain D (so that the union of the two boxes matters)"""
    h, w = shape
    cx, cy = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
    a, b, theta = rng.uniform(2, 14), rng.uniform(2, 9), rng.uniform(0, np.pi)
    original = clip(rotated_rectangle(cx, cy, a, b, theta) + rng.uniform(-1.5, 1.5, (4, 2)), shape)
    centre = original.mean(axis=0)
    dilated = original.copy() if rng.random() < 0.4 else clip(centre + 1.3 * (original - centre), shape)
    if rng.random() < 0.5:
        rectangle = box_polygon(bounding_box(dilated), int(rng.integers(0, 4)), shape)
    else:
        rectangle = clip(rotated_rectangle(cx, cy, 1.6 * a, 0.7 * b, theta), shape)
    return original, dilated, rectangle


def make_case(rng, shape, n):
    """n regions [(O, D, R)] of int32 (x, y) tables and their main angles.  n == 3: a quadrilateral A, a region nested in A, and
    a neighbour B whose rectangle covers A (r and T and not o is non-empty).  n > 3 starts with: a single point (BB 1 x 1), a
    two-point polygon (1 x N), a collinear one (N x 1), a region on the top and left borders, one on the bottom and right
    borders, a comb of 48 vertices with D == O, a comb of 68 vertices, then A, its nested region and B; random regions after."""
    h, w = shape
    quad_a = np.array([(20, 28), (60, 26), (62, 46), (22, 48)], np.int32)
    nested = np.array([(30, 32), (40, 32), (40, 40), (30, 40)], np.int32)
    quad_b = np.array([(63, 27), (90, 29), (88, 47), (64, 45)], np.int32)
    trio = [(quad_a, clip(quad_a.mean(axis=0) + 1.2 * (quad_a - quad_a.mean(axis=0)), shape), box_polygon(bounding_box(quad_a), 3, shape)),
            (nested, nested.copy(), box_polygon(bounding_box(nested), 2, shape)),
            (quad_b, clip(quad_b.mean(axis=0) + 1.2 * (quad_b - quad_b.mean(axis=0)), shape),
             box_polygon(union_box(bounding_box(quad_a), bounding_box(quad_b)), 1, shape))]
    point = np.array([(5, 50)], np.int32)
    segment = np.array([(10, 52), (40, 52)], np.int32)
    collinear = np.array([(3, 10), (3, 20), (3, 30)], np.int32)
    top_left = np.array([(0, 0), (12, 0), (14, 7), (0, 6)], np.int32)
    bottom_right = np.array([(w - 1, h - 1), (w - 14, h - 1), (w - 12, h - 8), (w - 1, h - 9)], np.int32)
    comb48, comb68 = comb(20, 2, 8, 11, 12), comb(50, 13, 20, 23, 17)
    special = [(point, point.copy(), point.copy()), (segment, segment.copy(), segment.copy()),
               (collinear, collinear.copy(), collinear.copy()),
               (top_left, box_polygon(bounding_box(top_left), 2, shape), box_polygon(bounding_box(top_left), 4, shape)),
               (bottom_right, box_polygon(bounding_box(bottom_right), 2, shape), box_polygon(bounding_box(bottom_right), 4, shape)),
               (comb48, comb48.copy(), box_polygon(bounding_box(comb48), 0, shape)),
               (comb68, comb68.copy(), box_polygon(bounding_box(comb68), 2, shape))] + trio
    if n == 3:
        regions = list(trio)
    else:
        regions = [special[k] if n > 3 and k < len(special) else random_region(rng, shape) for k in range(n)]
    angles = [ANGLES[(k + int(rng.integers(0, len(ANGLES)))) % len(ANGLES)] for k in range(n)]
    return regions, angles


def case_rng(shape, n, seed, base=2_000_000):
    return np.random.default_rng(base + 1000 * n + 10 * shape[0] + seed)


def load_golden():
    """tests/golden/text_region_masks.npz -> (runs, direct rectangle calls) with their arrays in place"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'text_region_masks.npz'))
    flats = {k: z[k] for k in z.files if k != 'index'}

    def resolve(v):
        if isinstance(v, list) and len(v) == 3 and isinstance(v[1], list) and isinstance(v[2], str) and v[2] in flats:
            at, shape, dtype = v
            return flats[dtype][at:at + int(np.prod(shape))].reshape(shape)
        if isinstance(v, dict):
            return {k: resolve(x) for k, x in v.items()}
        if isinstance(v, list):
            return [resolve(x) for x in v]
        return v

    index = json.loads(str(z['index']))
    return [resolve(row) for row in index['runs']], [resolve(row) for row in index['rectangles']]
