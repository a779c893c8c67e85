"""Char binding restated in plain numpy and Python loops, independent of vkit_amd: the reference's
calculate_boxed_masks_intersected_ratio (vkit/pipeline/text_detection/page_text_region.py:189-227),
PageTextRegionStep.strtree_query_intersected_polygons (:899-925) and the binding of chars to precise text regions (:1160-1216).

What the reference asks of shapely's STRtree is restated as the envelope rule: ``STRtree.query(geometry)`` without a predicate
answers the tree geometries whose envelope intersects the query's envelope, and the geometries are built from the integer
``to_xy_pairs()``: closed integer rectangles, touching ones included (tests/test_shapely_strtree_optional.py checks the rule
where shapely imports).  The masks are ``Polygon.mask``: the integer positions (Python's round, half to even) as float32,
the box from round() of their minima and maxima, the self-relative points rounded after the minimum is subtracted, a closing
duplicate of the first point dropped (PointList.from_np_array), cv.fillPoly (oracle.fill_poly) into the box's shape.

``make_case(seed, kind)`` builds the polygons that tests/golden/make_char_binding_golden.py, tests/test_char_binding_restate.py
and tests/test_gpu_char_binding.py share: float64 (n, 2) arrays of smooth (x, y).
"""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

KINDS = ('seams', 'envelope', 'binding', 'raster', 'page')
GOLDEN_SEEDS = (0, 1)
GOLDEN = os.path.join(HERE, 'golden', 'char_binding.npz')

SEAM_WIDTHS = (1, 31, 32, 33, 64, 65, 97)
SEAM_DX = (0, 1, 31, 32, 33)
SEAM_DY = (0, 1)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------
def int_points(points):
    """Point.x / Point.y: Python's round of the smooth position -> int64 (n, 2)"""
    return np.array([[round(float(x)), round(float(y))] for x, y in np.asarray(points, np.float64).reshape(-1, 2)], np.int64)


def envelope(points):
    """(xmin, xmax, ymin, ymax) of the integer to_xy_pairs()"""
    xy = int_points(points)
    return int(xy[:, 0].min()), int(xy[:, 0].max()), int(xy[:, 1].min()), int(xy[:, 1].max())


def envelopes_meet(a, c):
    return a[0] <= c[1] and c[0] <= a[1] and a[2] <= c[3] and c[2] <= a[3]


def self_relative(points):
    """-> (box (up, down, left, right), int32 (m, 2) self-relative points): Polygon.bounding_box and
    Polygon.self_relative_polygon.to_np_array()"""
    smooth = int_points(points).astype(np.float32)
    x_min, x_max, y_min, y_max = smooth[:, 0].min(), smooth[:, 0].max(), smooth[:, 1].min(), smooth[:, 1].max()
    box = (round(float(y_min)), round(float(y_max)), round(float(x_min)), round(float(x_max)))
    smooth[:, 0] -= x_min
    smooth[:, 1] -= y_min
    relative = [(round(float(x)), round(float(y))) for x, y in smooth]
    if len(relative) > 2 and relative[0] == relative[-1]:
        relative.pop()
    return box, np.array(relative, np.int32).reshape(-1, 2)


def polygon_mask(points):
    """Polygon.mask -> (box (up, down, left, right), uint8 mat of the box's shape)"""
    import oracle as O
    box, relative = self_relative(points)
    return box, O.fill_poly((box[1] - box[0] + 1, box[3] - box[2] + 1), relative)


def intersected_counts(anchor, candidate):
    """:200-218 on two (box, mat) masks -> (intersected_area, anchor area, candidate area), ints"""
    (a_box, a_mat), (c_box, c_mat) = anchor, candidate
    up, down = max(a_box[0], c_box[0]), min(a_box[1], c_box[1])
    left, right = max(a_box[2], c_box[2]), min(a_box[3], c_box[3])
    anchor_area, candidate_area = int((a_mat > 0).sum()), int((c_mat > 0).sum())
    if up > down or left > right:
        return None, anchor_area, candidate_area
    a = a_mat[up - a_box[0]:down - a_box[0] + 1, left - a_box[2]:right - a_box[2] + 1]
    c = c_mat[up - c_box[0]:down - c_box[0] + 1, left - c_box[2]:right - c_box[2] + 1]
    return int((a & c).sum()), anchor_area, candidate_area


def intersected_ratio(anchor, candidate, use_candidate_as_base=False):
    """:189-227"""
    intersected_area, anchor_area, candidate_area = intersected_counts(anchor, candidate)
    if intersected_area is None:
        return 0.0
    base_area = candidate_area if use_candidate_as_base else anchor_area + candidate_area - intersected_area
    return intersected_area / base_area


class Case:
    """The polygons of one case with their masks and envelopes, made once."""

    def __init__(self, anchors, candidates):
        self.anchors, self.candidates = anchors, candidates
        self.anchor_masks = [polygon_mask(p) for p in anchors]
        self.candidate_masks = [polygon_mask(p) for p in candidates]
        self.anchor_envelopes = [envelope(p) for p in anchors]
        self.candidate_envelopes = [envelope(p) for p in candidates]

    def query(self, c):
        """sorted(strtree.query(candidate c))"""
        return [a for a in range(len(self.anchors)) if envelopes_meet(self.anchor_envelopes[a], self.candidate_envelopes[c])]

    @functools.lru_cache(maxsize=None)
    def pairs(self):
        """every answer of every candidate -> (pairs (candidate, anchor), counts (intersected, anchor, candidate area)), lists"""
        pairs, counts = [], []
        for c in range(len(self.candidates)):
            for a in self.query(c):
                intersected_area, anchor_area, candidate_area = intersected_counts(self.anchor_masks[a], self.candidate_masks[c])
                pairs.append((c, a))
                counts.append((intersected_area or 0, anchor_area, candidate_area))
        return pairs, counts

    @functools.lru_cache(maxsize=None)
    def ratios(self, use_candidate_as_base=True):
        return [intersected_ratio(self.anchor_masks[a], self.candidate_masks[c], use_candidate_as_base) for c, a in self.pairs()[0]]

    @functools.lru_cache(maxsize=None)
    def bind(self):
        """:1176-1205 -> the bound anchor of every candidate (-1: none)"""
        bound = []
        for c in range(len(self.candidates)):
            best, ratio_max = None, 0
            for a in self.query(c):
                ratio = intersected_ratio(self.anchor_masks[a], self.candidate_masks[c], True)
                if ratio > ratio_max:
                    ratio_max, best = ratio, a
            bound.append(-1 if best is None else best)
        return bound

    def infos(self):
        """:1207-1216 -> [(region index, [char indices])]"""
        bound = self.bind()
        return [(a, [c for c, b in enumerate(bound) if b == a]) for a in range(len(self.anchors)) if a in bound]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def rect(left, up, w, h):
    """the rectangle of w x h pixels at (left, up)"""
    return np.array([(left, up), (left + w - 1, up), (left + w - 1, up + h - 1), (left, up + h - 1)], np.float64)


def comb(left, up, tooth, height, teeth):
    """a comb of 4 * teeth vertices: `teeth` teeth of `tooth` columns, `height` rows tall, standing on the closing edge"""
    points = []
    for k in range(teeth):
        x = left + 2 * k * tooth
        points += [(x, up + height), (x, up), (x + tooth - 1, up), (x + tooth - 1, up + height)]
    return np.array(points, np.float64)


def jittered(rng, left, up, w, h):
    """a convex-ish hexagon inside the w x h box at (left, up) that reaches all four sides"""
    if w < 3 or h < 3:
        return rect(left, up, w, h)
    xs = sorted(int(v) for v in rng.integers(1, w - 1, 2))
    ys = sorted(int(v) for v in rng.integers(1, h - 1, 2))
    return np.array([(left + xs[0], up), (left + w - 1, up + ys[0]), (left + w - 1, up + ys[1]), (left + xs[1], up + h - 1),
                     (left, up + ys[1]), (left, up + ys[0])], np.float64)


def _seams(rng):
    anchors, candidates = [], []
    cell = 0
    for w in SEAM_WIDTHS:
        for dx in SEAM_DX:
            for dy in SEAM_DY:
                left, up = 300 * (cell % 10) + int(rng.integers(0, 64)), 60 * (cell // 10)
                cell += 1
                candidates.append(jittered(rng, left, up, w, 5 + dy))
                anchors.append(jittered(rng, left + dx, up + dy, w + int(rng.integers(2, 40)), 7))
                # ... and the anchor to the LEFT of the candidate by the same shift (a negative word offset)
                candidates.append(jittered(rng, left + dx, up + 20 + dy, w, 6))
                anchors.append(jittered(rng, left, up + 20, w + dx + int(rng.integers(0, 3)), 5))
    base = 60 * (cell // 10 + 1)
    # an intersection window of 1 x 1: two boxes that share one corner pixel
    candidates.append(rect(10, base, 11, 11))
    anchors.append(rect(20, base + 10, 11, 11))
    # a window that starts mid-word and ends on a word's last bit: columns 13 .. 63 of a candidate of 97
    candidates.append(jittered(rng, 200, base, 97, 9))
    anchors.append(rect(213, base + 2, 51, 4))
    # ... and one that starts on a word's first bit and ends mid-word, two words in
    candidates.append(jittered(rng, 400, base, 97, 9))
    anchors.append(rect(432, base - 3, 40, 8))
    return anchors, candidates


def _envelope(rng):
    j = int(rng.integers(0, 5))
    anchors = [rect(10, 10 + j, 10, 10),                                       # 0: columns 10 .. 19
               rect(10, 40 + j, 10, 10),                                       # 1
               np.array([(112, 12), (112, 3), (103, 12)], np.float64),         # 2: a triangle in the far corner of its box
               rect(200, 10, 40 + j, 30),                                      # 3: the outer of a nested pair
               rect(300, 10, 8, 8)]                                            # 4: met by nobody
    candidates = [rect(19, 12 + j, 6, 5),                                      # touches anchor 0 on column 19
                  rect(20, 42 + j, 6, 5),                                      # one pixel from anchor 1: no answer
                  np.array([(100, 0), (110, 0), (100, 10)], np.float64),       # envelopes overlap anchor 2's, no shared pixel
                  rect(210, 15, 7 + j, 6),                                     # nested in anchor 3
                  rect(5, 19 + j, 8, 4),                                       # touches anchor 0 on its last row
                  rect(500, 500, 3, 3)]                                        # meets nothing
    return anchors, candidates


def _binding(rng):
    j = int(rng.integers(0, 4))
    anchors = [rect(0, 0, 40, 20), rect(0, 0, 40, 20),                         # 0, 1: equal ratios -> 0
               rect(100, 0, 12, 20), rect(108, 0, 30, 20), rect(104, 0, 10, 20),   # 2, 3, 4: the second of three wins
               np.array([(212, 12), (212, 3), (203, 12)], np.float64),         # 5: met, never shared
               rect(300, 0, 25, 25),                                           # 6: a region with no char
               rect(400, 0, 30, 12 + j)]                                       # 7
    candidates = [rect(5 + j, 4, 9, 9),                                        # -> 0 (ties with 1)
                  rect(106, 5, 10, 8),                                         # ratios 0.6, 0.8, 0.8 -> 3 (the second; 4 ties later)
                  np.array([(200, 0), (210, 0), (200, 10)], np.float64),       # unbound: envelopes meet, ratio 0.0
                  rect(600, 600, 5, 5),                                        # unbound: no answer at all
                  rect(405, 2, 6, 6), rect(415, 3, 6, 6), rect(398, 5, 6, 6)]  # -> 7, in char order
    return anchors, candidates


def _raster(rng):
    j = int(rng.integers(0, 3))
    shapes = [np.array([(5, 5)], np.float64),                                                  # one point
              np.array([(3, 8), (14, 2)], np.float64),                                         # two points
              np.array([(2, 12), (7, 12), (16, 12)], np.float64),                              # collinear, flat
              np.array([(1, 1), (4, 4), (9, 9)], np.float64),                                  # collinear, slanted
              comb(0, 0, 1, 9, 17),                                                            # a comb of 68 vertices: 34 crossings a row
              np.array([(0, 0), (15, 11), (15, 0), (0, 11)], np.float64),                      # self-crossing (even-odd)
              np.array([(0.5, 1.5), (12.5, 2.5), (11.5, 9.5), (2.5, 10.5)], np.float64),       # .5: half to even both ways
              np.array([(1.5, 0.49), (13.51, 3.5), (8.5, 12.5)], np.float64),
              np.array([(-7, -3), (6, -5), (9, 8), (-4, 6)], np.float64),                      # negative coordinates
              np.array([(-20.5, -11.5), (-2.5, -9.5), (-6.5, -0.5)], np.float64),
              np.array([(2, 2), (12, 3), (10, 11), (2, 2)], np.float64),                       # a closing duplicate
              np.array([(0, 0), (33 + j, 0), (33 + j, 6), (20, 6), (20, 3), (10, 3), (10, 6), (0, 6)], np.float64)]   # concave
    assert len(shapes[4]) == 68
    anchors, candidates = [], []
    for k, shape in enumerate(shapes):
        anchors.append(shape + (40 * (k % 4) + int(rng.integers(0, 6)), 30 * (k // 4)))
        candidates.append(shape + (40 * ((k + 1) % 4) + int(rng.integers(0, 9)) - 4, 30 * (k // 4) + int(rng.integers(0, 5)) - 2))
        candidates.append(shape[::-1] + (40 * (k % 4) + int(rng.integers(0, 6)), 30 * (k // 4) + 1))
    return anchors, candidates


def _page(rng):
    """300 chars against 5 regions; a region of 1 x 2000 and one of 600 x 3 against 40 chars each"""
    anchors, candidates = [], []
    for r in range(5):
        up = 60 * r
        anchors.append(np.array([(10, up + int(rng.integers(0, 6))), (1000, up + int(rng.integers(0, 10))),
                                 (1005, up + 40 + int(rng.integers(0, 6))), (8, up + 44)], np.float64))
        for k in range(60):
            left = 14 + 16 * k + int(rng.integers(0, 3))
            top = up + 4 + int(rng.integers(0, 30))
            w, h = int(rng.integers(6, 15)), int(rng.integers(8, 30))
            candidates.append(np.array([(left + rng.random() * 2, top + rng.random() * 2), (left + w, top + rng.random() * 3),
                                        (left + w - rng.random() * 2, top + h), (left, top + h - rng.random() * 2)], np.float64))
    anchors.append(rect(0, 400, 2000, 1))
    anchors.append(rect(1100, 0, 3, 600))
    for k in range(40):
        candidates.append(jittered(rng, 50 * k + int(rng.integers(0, 30)), 395 + int(rng.integers(0, 4)), int(rng.integers(3, 40)), 9))
        candidates.append(jittered(rng, 1095 + int(rng.integers(0, 6)), 15 * k, 12, int(rng.integers(3, 14))))
    return anchors, candidates


def make_case(seed, kind):
    """-> (anchors, candidates): lists of float64 (n, 2) arrays of smooth (x, y)"""
    rng = np.random.default_rng([KINDS.index(kind), int(seed), 20261021])
    anchors, candidates = {'seams': _seams, 'envelope': _envelope, 'binding': _binding, 'raster': _raster, 'page': _page}[kind](rng)
    return [np.asarray(p, np.float64) for p in anchors], [np.asarray(p, np.float64) for p in candidates]


# ---- the golden file ---------------------------------------------------------------------------------------------------
def load_golden(path=GOLDEN):
    """-> [dict(kind, seed, anchors, candidates, pairs, counts, ratio, ratio_union, bound, infos)] as written by
    tests/golden/make_char_binding_golden.py"""
    data = np.load(path)
    index = json.loads(str(data['index']))
    runs = []
    for entry in index['runs']:
        run = dict(kind=entry['kind'], seed=entry['seed'], infos=[(a, list(chars)) for a, chars in entry['infos']])
        for name in ('anchors', 'candidates'):
            run[name] = [data['points'][at:at + n].copy() for at, n in entry[name]]
        for name, key in (('pairs', 'int'), ('counts', 'int'), ('bound', 'int'), ('ratio', 'float'), ('ratio_union', 'float')):
            at, shape = entry[name]
            run[name] = data[key][at:at + int(np.prod(shape))].reshape(shape).copy()
        runs.append(run)
    return runs
