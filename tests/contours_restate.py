"""cv.findContours(mask * 255, RETR_TREE, method) filtered to the contours whose hierarchy parent is -1, restated twice in
numpy / plain Python from the published algorithm (Suzuki & Abe 1985; the trace is OpenCV's icvFetchContour):

    contours_scan   the raster scan itself: border following with pixel marks (NBD, -NBD on a right edge), LNBD and the parent
                    table; hole borders are followed for their marks, only the outer borders whose parent is the frame are kept.
    contours_label  labelling: 8-connected foreground and 4-connected background components, a foreground component is kept when
                    the background pixel west of its raster-first pixel lies outside the plane or belongs to the background
                    region that reaches the plane's edge; kept components in raster order of that pixel, each traced on the
                    untouched plane.

Both return a list of int32 (k, 2) arrays of (x, y), in order.  Direction codes 0..7 are E, NE, N, NW, W, SW, S, SE, y down.
Unpinned against a cv2 binary (tests/test_cv2_contours_optional.py compares where cv2 imports)."""
import numpy as np

CHAIN_APPROX_NONE, CHAIN_APPROX_SIMPLE = 1, 2
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)


def _check_method(method):
    if method not in (CHAIN_APPROX_NONE, CHAIN_APPROX_SIMPLE):
        raise ValueError(f'unsupported cv.findContours method {method}')


# ---- first restatement: the raster scan with marks ---------------------------------------------------------------------------
def _follow(f, x0, y0, is_hole, nbd, method):
    """follow one border from (x0, y0) of the padded plane f, leave its marks, -> its points in padded coordinates"""
    s_end = s = 0 if is_hole else 4
    while True:
        s = (s - 1) & 7
        if f[y0 + DY[s]][x0 + DX[s]] != 0 or s == s_end:
            break
    if s == s_end:
        f[y0][x0] = -nbd
        return [(x0, y0)]
    x1, y1 = x0 + DX[s], y0 + DY[s]
    x3, y3 = x0, y0
    prev_s = s ^ 4
    points = []
    while True:
        east_was_zero = False
        while True:
            s = (s + 1) & 7
            x4, y4 = x3 + DX[s], y3 + DY[s]
            if f[y4][x4] != 0:
                break
            if s == 0:
                east_was_zero = True
        if method == CHAIN_APPROX_NONE or s != prev_s:
            points.append((x3, y3))
            prev_s = s
        if east_was_zero:
            f[y3][x3] = -nbd
        elif f[y3][x3] == 1:
            f[y3][x3] = nbd
        if (x4, y4) == (x0, y0) and (x3, y3) == (x1, y1):
            return points
        x3, y3 = x4, y4
        s = (s + 4) & 7


def contours_scan(mask, method=CHAIN_APPROX_SIMPLE):
    _check_method(method)
    mask = np.asarray(mask)
    h, w = mask.shape
    f = [[0] * (w + 2) for _ in range(h + 2)]
    for y, x in zip(*np.nonzero(mask > 0)):
        f[y + 1][x + 1] = 1
    nbd = 1
    is_hole_border, parent = {1: True}, {1: 0}          # border 1 is the frame
    out = []
    for y in range(1, h + 1):
        row = f[y]
        lnbd = 1
        for x in range(1, w + 1):
            v = row[x]
            if v == 0:
                continue
            hole = None
            if v == 1 and row[x - 1] == 0:
                hole = False
            elif v >= 1 and row[x + 1] == 0:
                hole = True
                if v > 1:
                    lnbd = v
            if hole is not None:
                nbd += 1
                is_hole_border[nbd] = hole
                parent[nbd] = lnbd if is_hole_border[lnbd] != hole else parent[lnbd]
                points = _follow(f, x, y, hole, nbd, method)
                if not hole and parent[nbd] == 1:
                    out.append(np.array(points, np.int32).reshape(-1, 2) - 1)
            v = row[x]
            if v != 1:
                lnbd = abs(v)
    return out


# ---- second restatement: labelling, the start test, the trace ---------------------------------------------------------------
def trace(fg, x0, y0, method):
    """the outer border of the component whose raster-first pixel is (x0, y0), on the boolean plane fg"""
    h, w = fg.shape

    def is_set(x, y):
        return 0 <= x < w and 0 <= y < h and bool(fg[y, x])

    s = 4
    while True:
        s = (s - 1) & 7
        if is_set(x0 + DX[s], y0 + DY[s]) or s == 4:
            break
    if not is_set(x0 + DX[s], y0 + DY[s]):
        return np.array([(x0, y0)], np.int32)
    p0, p1 = (x0, y0), (x0 + DX[s], y0 + DY[s])
    p3, prev_s = p0, s ^ 4
    points = []
    while True:
        while True:
            s = (s + 1) & 7
            p4 = (p3[0] + DX[s], p3[1] + DY[s])
            if is_set(*p4):
                break
        if method == CHAIN_APPROX_NONE or s != prev_s:
            points.append(p3)
            prev_s = s
        if p4 == p0 and p3 == p1:
            return np.array(points, np.int32)
        p3, s = p4, (s + 4) & 7


def contours_label(mask, method=CHAIN_APPROX_SIMPLE):
    from scipy import ndimage
    _check_method(method)
    fg = np.asarray(mask) > 0
    h, w = fg.shape
    fg_label, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    bg_label, _ = ndimage.label(~np.pad(fg, 1))                        # 4-connected; the pad is the frame
    frame = bg_label[0, 0]
    labels, first = np.unique(fg_label.ravel(), return_index=True)     # first: the raster-first pixel of every label
    out = []
    for label, index in sorted(zip(labels, first), key=lambda t: t[1]):
        if label == 0:
            continue
        y, x = divmod(int(index), w)
        if bg_label[y + 1, x] == frame:                                 # (x - 1, y) in padded coordinates
            out.append(trace(fg, x, y, method))
    return out


contours = contours_scan      # what the GPU tests compare with: plain Python, no scipy


def same_contours(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and (a == b).all(), (a.tolist(), b.tolist())


def random_mask(rng, max_h=39, max_w=39, blobs=False):
    h, w = int(rng.integers(1, max_h + 1)), int(rng.integers(1, max_w + 1))
    density = float(rng.uniform(0.05, 0.95))
    mask = rng.random((h, w)) < density
    if blobs:                                                           # dilate a sparse plane into blobs
        seeds = rng.random((h, w)) < density * 0.08
        mask = np.zeros((h, w), bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                shifted = np.zeros((h, w), bool)
                ys, xs = np.nonzero(seeds)
                ys, xs = ys + dy, xs + dx
                ok = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
                shifted[ys[ok], xs[ok]] = True
                mask |= shifted
    return mask.astype(np.uint8)
