"""numpy + oracle restatement of the default char-heatmap engine (reference: engine/char_heatmap/default.py:93-180).

cv.getPerspectiveTransform, cv.warpPerspective (float32 path) and cv.fillPoly are the oracle's
(oracle.get_perspective_transform / warp_perspective / fill_poly); the fills, Mask.from_polygons and the numpy tail are
numpy as the reference runs them, the box extraction asserts and the boolean indexing included, so a char whose box is not
inside the page raises what the reference raises.  Chars are float64 (4, 2) smooth (x, y) arrays."""
import json
import os

import numpy as np

import oracle as O

DEFAULTS = dict(factor=2.25, radius=25, preserving=0.9, weight=0.4)


def template(radius, factor):
    """build_np_distance + generate_np_gaussian_map, the reference's expressions (float32 throughout)."""
    side = radius * 2 + 1
    off = np.abs(np.arange(side, dtype=np.float32) - radius)
    dist = np.sqrt(np.square(np.repeat(off[:, None], side, axis=1)) + np.square(np.repeat(off[None, :], side, axis=0)))
    norm = dist / radius
    gauss = np.exp(-0.5 * np.square(factor * norm))
    end = side - 1
    points = np.asarray([(0, 0), (end, 0), (end, end), (0, end)], dtype=np.float32)
    return gauss, points


def _extract(mat, up, down, left, right):
    """Box.extract_np_array (element/box.py:239-242)"""
    assert 0 <= up <= down <= mat.shape[0]
    assert 0 <= left <= right <= mat.shape[1]
    return mat[up:down + 1, left:right + 1]


def _fill(page, box, value, np_mask, keep_max):
    """Polygon.fill_score_map(page, ScoreMap(value, box), keep_*_value) -> Box.fill_np_array -> opt.fill_np_array"""
    up, down, left, right = box
    shape = (down - up + 1, right - left + 1)
    mat = page
    if page.shape != shape:
        mat = _extract(page, up, down, left, right)
    if value.shape != mat.shape:
        assert value.shape == page.shape
        value = _extract(value, up, down, left, right)
    sub = mat[np_mask]
    v = value[np_mask]
    np.putmask(sub, (sub < v) if keep_max else (sub > v), v)
    mat[np_mask] = sub


def char_geometry(quad):
    """(integer points relative to the box as float32 (4, 2), box (up, down, left, right)): Polygon.internals."""
    pts = np.asarray([[round(x), round(y)] for x, y in np.asarray(quad, np.float64).reshape(4, 2).tolist()], np.float32)
    y_min, y_max = pts[:, 1].min(), pts[:, 1].max()
    x_min, x_max = pts[:, 0].min(), pts[:, 0].max()
    rel = pts.copy()
    rel[:, 0] -= x_min
    rel[:, 1] -= y_min
    return rel, (round(y_min), round(y_max), round(x_min), round(x_max))


def run(quads, shape, radius=25, factor=2.25, preserving=0.9, weight=0.4):
    """The engine: dict of score + the six debug planes, or raises the reference's exception."""
    gauss, src = template(radius, factor)
    h, w = shape
    score_max = np.zeros(shape, np.float32)
    score_min = np.ones(shape, np.float32)
    count = np.zeros(shape, np.int32)
    rasters = []
    for quad in quads:
        rel, box = char_geometry(quad)
        up, down, left, right = box
        bh, bw = down - up + 1, right - left + 1
        H = O.get_perspective_transform(src, rel)
        warped = O.warp_perspective(gauss, H, (bw, bh))
        np_mask = O.fill_poly((bh, bw), rel.astype(np.int32)).astype(bool)
        _fill(score_max, box, warped, np_mask, True)
        _fill(score_min, box, warped, np_mask, False)
        rasters.append((box, np_mask))
    for (up, down, left, right), np_mask in rasters:       # Mask.from_polygons(shape, polygons, INTERSECT)
        _extract(count, up, down, left, right)[np_mask] += 1
    overlapped = (count > 1).astype(np.uint8)
    preserving_mask = score_max >= preserving
    neutralized = (overlapped.astype(bool) & ~preserving_mask).astype(np.uint8)
    delta = np.clip(score_max - score_min, 0.0, 1.0)
    nscore = score_max.copy()
    nscore[neutralized > 0] = delta[neutralized > 0]
    score = (1 - weight) * score_max + weight * nscore
    assert score.dtype == np.float32 and delta.dtype == np.float32
    return dict(score=score, score_map_max=score_max, score_map_min=score_min, char_overlapped_mask=overlapped,
                char_neutralized_score_map=delta, neutralized_mask=neutralized, neutralized_score_map=nscore)


DEBUG_NAMES = ('score_map_max', 'score_map_min', 'char_overlapped_mask', 'char_neutralized_score_map', 'neutralized_mask',
               'neutralized_score_map')


def config_of(case):
    return {k: case[k] for k in DEFAULTS}


def load_golden():
    """tests/golden/char_heatmap.npz as a list of case dicts with their arrays in place (make_char_heatmap_golden.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'char_heatmap.npz'))
    flats = {k: z[k] for k in z.files if k != 'index'}
    key = {'float64': 'f64', 'uint8': 'u8', 'float32': 'f32'}
    cases = []
    for row in json.loads(str(z['index'])):
        case = {}
        for k, v in row.items():
            if isinstance(v, list) and len(v) == 3 and isinstance(v[1], list) and v[2] in key:
                at, shape, dtype = v
                case[k] = flats[key[dtype]][at:at + int(np.prod(shape))].reshape(shape)
            else:
                case[k] = v
        cases.append(case)
    return cases


def text_line_quads(rng, shape, n_chars, height=(18, 30), step=(0.8, 1.0), tilt=0.15, jitter=0.08):
    """About ``n_chars`` chars as text lines over a page: rows of chars of one height, each advanced by ``step`` times its
    width (below 1: touching and overlapping neighbours), slightly rotated and in mild perspective, boxes inside the page.
    float64 (N, 4, 2)."""
    h, w = shape
    out = []
    y = 1.0
    while len(out) < n_chars and y < h - 2:
        ch = rng.uniform(*height)
        cy = y + ch / 2
        x = 1.0 + rng.uniform(0, ch)
        while len(out) < n_chars and x + ch < w - 1:
            cw = ch * rng.uniform(0.6, 1.0)
            a = rng.uniform(-tilt, tilt)
            base = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64) * (cw / 2, ch / 2)
            rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            q = base @ rot.T + rng.uniform(-jitter, jitter, (4, 2)) * ch + (x + cw / 2, cy)
            out.append(q)
            x += cw * rng.uniform(*step)
        y += ch * rng.uniform(0.85, 1.1)
    q = np.round(np.asarray(out, np.float64).reshape(-1, 4, 2), 3)
    q[:, :, 0] = np.clip(q[:, :, 0], 0, w - 1)
    q[:, :, 1] = np.clip(q[:, :, 1], 0, h - 1)
    return q
