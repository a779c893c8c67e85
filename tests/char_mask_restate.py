"""numpy + oracle restatement of the external_ellipse char-mask engine (reference: engine/char_mask/external_ellipse.py:
104-220) and of the page labels PageDistortionStep builds from it (pipeline/text_detection/page_distortion.py:225-300).

cv.getPerspectiveTransform and cv.warpPerspective are the oracle's (oracle.get_perspective_transform / warp_perspective,
with cv2's rule that a dsize with a zero side means the source size); everything else is numpy as the reference runs it,
np.matmul of affine_np_points included.  Chars are float64 (4, 2) smooth (x, y) arrays."""
import math

import numpy as np

import oracle as O

ERRORS = {1: RuntimeError, 2: AssertionError, 3: ValueError, 4: OverflowError}


def template(L):
    R = math.ceil(L / math.sqrt(2))
    side = 2 * R + 1
    off = np.abs(np.arange(side, dtype=np.float32) - R)
    dist = np.sqrt(np.square(np.repeat(off[:, None], side, axis=1)) + np.square(np.repeat(off[None, :], side, axis=0)))
    mask = (dist <= R).astype(np.uint8)
    pad = (side - L) // 2
    b, e = pad, pad + L - 1
    char_pts = np.asarray([(b, b), (e, b), (e, e), (b, e)], np.float32)
    ext_pts = np.asarray([(0, 0), (side - 1, 0), (side - 1, side - 1), (0, side - 1)], np.float32)
    return mask, char_pts, ext_pts


def warp(src, M, dsize):
    w, h = int(dsize[0]), int(dsize[1])
    if w <= 0 or h <= 0:
        h, w = src.shape[:2]
    return O.warp_perspective(src, M, (w, h))


def char_mask(quad, L, bounds):
    """One char: (status, box (up, down, left, right), trimmed warped template or None).  ``bounds`` = (up, down, left,
    right).  status 0 placed; else the index of ERRORS the reference raises."""
    mask, char_pts, ext_pts = template(L)
    quad = np.asarray(quad, np.float64).reshape(4, 2)
    # Polygon.internals.np_self_relative_points: PointTuple.to_smooth_np_array holds the INTEGER points (round(smooth),
    # element/point.py:251) as float32, minus their min
    rel = np.asarray([[round(x), round(y)] for x, y in quad.tolist()], dtype=np.float32)
    rel = rel - rel.min(axis=0)
    H1 = O.get_perspective_transform(char_pts, rel)
    pts = np.concatenate((ext_pts.T, np.ones((1, 4), np.float32)))
    res = np.matmul(H1, pts)
    tp = (res[:2, :] / res[2, :]).T
    y_off, x_off = tp[:, 1].min(), tp[:, 0].min()
    tp[:, 1] -= y_off
    tp[:, 0] -= x_off
    tp = tp.astype(np.float32)
    H2 = O.get_perspective_transform(ext_pts, tp)
    try:
        th, tw = math.ceil(tp[:, 1].max()), math.ceil(tp[:, 0].max())
    except ValueError:
        return 3, None, None
    except OverflowError:
        return 4, None, None
    if max(abs(th), abs(tw)) >= 1 << 30:
        return 4, None, None
    warped = warp(mask, H2, (tw, th))
    up = round(float(quad[:, 1].min()) + y_off)
    left = round(float(quad[:, 0].min()) + x_off)
    down, right = up + th - 1, left + tw - 1
    bu, bd, bl, br = bounds
    tu, td, tl, tr = 0, th - 1, 0, tw - 1
    if up < bu:
        tu, up = bu - up, bu
    if down > bd:
        td, down = td - (down - bd), bd
    if left < bl:
        tl, left = bl - left, bl
    if right > br:
        tr, right = tr - (right - br), br
    trimmed = warped[tu:td + 1, tl:tr + 1]
    if trimmed.shape != (down - up + 1, right - left + 1):
        return 1, None, None
    if trimmed.shape[0] == 0 or trimmed.shape[1] == 0:
        return 2, None, None
    return 0, (up, down, left, right), trimmed


def run(quads, L, shape, bounds=None):
    """The engine: (combined mask, [(box, mat)] per char), or raises the reference's exception."""
    h, w = shape
    combined = np.zeros(shape, np.uint8)
    out = []
    for i, quad in enumerate(quads):
        status, box, mat = char_mask(quad, L, bounds[i] if bounds is not None else (0, h - 1, 0, w - 1))
        if status:
            raise ERRORS[status]()
        up, down, left, right = box
        combined[up:down + 1, left:right + 1][mat > 0] = 1
        out.append((box, mat))
    return combined, out


def height_map(quads, L, shape, heights):
    """PageDistortionStep's char height map with the ellipse engine: char masks filled from large to small height."""
    _, chars = run(quads, L, shape)
    score = np.zeros(shape, np.float32)
    for idx in reversed(np.asarray(heights).argsort()):
        (up, down, left, right), mat = chars[idx]
        score[up:down + 1, left:right + 1][mat > 0] = np.float32(heights[idx])
    return score


def load_golden():
    """tests/golden/char_mask.npz as a list of case dicts with their arrays in place (make_char_mask_golden.py)."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'char_mask.npz'))
    flats = {k: z[k] for k in z.files if k != 'index'}
    key = {'float64': 'f64', 'int32': 'i32', 'uint8': 'u8', 'float32': 'f32'}
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
