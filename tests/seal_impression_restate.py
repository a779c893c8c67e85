"""numpy-plus-oracle restatement of fill_text_line_to_seal_impression (reference: engine/seal_impression/
text_line_slot_filler.py:28-205) for the tests of csrc/seal_fill.hip and of vkit_amd.engine.seal_impression, and the synthetic
cases those tests and tests/golden/make_seal_impression_golden.py share.  Tests only: the product never imports this.

A case is plain data (``make_case``):
    seal      h, w, alpha, slots [{height, aspect, chars [[angle, up_y, up_x, down_y, down_x], ...]}], internal_box or None
    indices   the text-line slot index of every text line
    lines     [{height, width, interp, chars [{box [up, down, left, right], score float32 | None, image uint8, ref_h, ref_w}]}]
    internal  None | {height, width, score float32 | None, mask uint8, chars [{box, ref_h, ref_w}]}
``fill(case)`` walks it as the reference does: per char the glyph resized (oracle.resize; clipped to [0, 1] for a score map,
``(mask * 255) -> > 0`` for a mask), laid into a plane of the line's height, rotated by ``angle - 270`` (RotateState's matrix in
float32, oracle.warp_affine), filled at ``point_up - rotated point_up`` keeping the maximum unless out of bound; then the
internal line's overwrite and ``map * alpha / max``.
"""
import json
import math
import os

import numpy as np

import oracle as O

INTERPOLATIONS = dict(NEAREST_EXACT=6, LINEAR_EXACT=5, CUBIC=2, LANCZOS4=4, AREA=3)


def py_round_point(value):
    return round(float(value))


def rotate_state(angle, shape):
    """RotateState (mechanism/distortion/geometric/affine.py): (float32 2 x 3 forward matrix, (dst_width, dst_height))"""
    height, width = shape
    rad = math.radians(angle % 360)
    sin, cos = math.sin, math.cos
    if rad <= math.pi / 2:
        shift_x, shift_y = height * sin(rad), 0
        dst_width = height * sin(rad) + width * cos(rad)
        dst_height = height * cos(rad) + width * sin(rad)
    elif rad <= math.pi:
        local = rad - math.pi / 2
        shift_x = width * sin(local) + height * cos(local)
        shift_y = height * sin(local)
        dst_width = shift_x
        dst_height = shift_y + width * cos(local)
    elif rad < math.pi * 3 / 2:
        local = rad - math.pi
        shift_x = width * cos(local)
        shift_y = width * sin(local) + height * cos(local)
        dst_width = shift_x + height * sin(local)
        dst_height = shift_y
    else:
        local = rad - math.pi * 3 / 2
        shift_x, shift_y = 0, width * cos(local)
        dst_width = width * sin(local) + height * cos(local)
        dst_height = shift_y + height * sin(local)
    mat = np.asarray([(cos(rad), -sin(rad), math.ceil(shift_x)), (sin(rad), cos(rad), math.ceil(shift_y))], dtype=np.float32)
    return mat, (math.ceil(dst_width), math.ceil(dst_height))


def rotate_branch(angle):
    """which of RotateState's four branches ``angle`` takes"""
    rad = math.radians(angle % 360)
    return 0 if rad <= math.pi / 2 else 1 if rad <= math.pi else 2 if rad < math.pi * 3 / 2 else 3


def move_points(mat, xy):
    """affine_np_points: float32 (n, 2) (x, y) through the float32 matrix"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    homogeneous = np.concatenate((xy.transpose(), np.ones((1, xy.shape[0]), dtype=np.float32)))
    return np.matmul(mat, homogeneous).transpose()


def glyph_mask(image):
    return (image > 0) if image.ndim == 2 else np.any(image > 0, axis=2)


def resized_glyph(char, interp, shape):
    """the char's glyph as float32 of ``shape``: the score map way or, without one, the mask way"""
    if char['score'] is not None:
        score = char['score']
        if score.shape != shape:
            score = np.clip(O.resize(score, shape, interp), 0.0, 1.0)
        return score.astype(np.float32)
    mask = glyph_mask(char['image']).astype(np.uint8)
    if mask.shape != shape:
        mask = (O.resize(mask * np.uint8(255), shape, interp) > 0).astype(np.uint8)
    return mask.astype(np.float32)


def char_plan(line, slot, char, char_slot, factor):
    """(resized width, char polygon (4, 2) float64 (x, y), angle) of one char"""
    up, down, _left, _right = char['box']
    glyph_width = char['image'].shape[1]
    resized_width = max(1, round(factor * glyph_width))
    box_height = down - up + 1
    p_up, p_down = up, down
    if box_height < char['ref_h']:
        half_inc = (char['ref_h'] - box_height) / 2
        p_up, p_down = p_up - half_inc, p_down + half_inc
    p_left, p_right = 0, resized_width - 1
    ref_char_width = factor * char['ref_w']
    if resized_width < ref_char_width:
        half_inc = (ref_char_width - resized_width) / 2
        p_left, p_right = p_left - half_inc, p_right + half_inc
    polygon = np.array([(p_left, p_up), (p_right, p_up), (p_right, p_down), (p_left, p_down)], np.float64)
    return resized_width, polygon, char_slot[0] - 270


def rotated_polygon(mat, polygon, nop):
    """Polygon through rotate.distort without clipping: float32 products become the smooth positions; a closing duplicate goes"""
    if nop:
        return polygon.copy()
    moved = move_points(mat, polygon.astype(np.float32)).astype(np.float64)
    ints = np.array([[round(float(v)) for v in row] for row in moved])
    if len(moved) > 2 and (ints[0] == ints[-1]).all():
        moved = moved[:-1]
    return moved


def internal_polygons(internal, box, shape):
    """TextLine.to_char_polygons of the shifted horizontal internal text line"""
    height, width = shape
    out = []
    for char in internal['chars']:
        up, down, left, right = char['box']
        up, down, left, right = up + box[0], down + box[0], left + box[2], right + box[2]
        c_h, c_w = down - up + 1, right - left + 1
        if c_h < char['ref_h']:
            half_inc = (char['ref_h'] - c_h) / 2
            up, down = max(0, up - half_inc), min(height - 1, down + half_inc)
        if c_w < char['ref_w']:
            half_inc = (char['ref_w'] - c_w) / 2
            left, right = max(0, left - half_inc), min(width - 1, right + half_inc)
        out.append(np.array([(left, up), (right, up), (right, down), (left, down)], np.float64))
    return out


def fill(case, stats=None):
    """-> (score map float32 (h, w), char polygons [(n, 2) float64 (x, y)]); ``stats``: a dict that counts chars seen / placed"""
    seal = case['seal']
    height, width = seal['h'], seal['w']
    score_map = np.zeros((height, width), np.float32)
    polygons = []
    for slot_index, line in zip(case['indices'], case['lines']):
        if slot_index >= len(seal['slots']):
            break
        slot = seal['slots'][slot_index]
        ref_h = ref_w = 0
        for char in line['chars']:
            if char['ref_h'] > ref_h:
                ref_h, ref_w = char['ref_h'], char['ref_w']
        assert ref_h > 0 and ref_w > 0
        factor = slot['aspect'] / (ref_w / ref_h)
        for k, char in enumerate(line['chars']):
            if k >= len(slot['chars']):
                break
            char_slot = slot['chars'][k]
            resized_width, polygon, angle = char_plan(line, slot, char, char_slot, factor)
            up, down = char['box'][0], char['box'][1]
            plane = np.zeros((line['height'], resized_width), np.float32)
            plane[up:down + 1, :] = resized_glyph(char, line['interp'], (down - up + 1, resized_width))
            mat, dsize = rotate_state(angle, plane.shape)
            nop = angle == 0
            rotated = plane if nop else O.warp_affine(plane, mat, dsize)
            # the point goes in by its INTEGER position (PointTuple.to_smooth_np_array)
            point = np.array([(py_round_point(resized_width / 2), 0)], np.float32)
            moved = point if nop else move_points(mat, point)
            point_x, point_y = py_round_point(moved[0, 0]), py_round_point(moved[0, 1])
            dst_up = py_round_point(char_slot[1]) - point_y
            dst_left = py_round_point(char_slot[2]) - point_x
            if stats is not None:
                stats['chars'] = stats.get('chars', 0) + 1
            if dst_up < 0 or dst_up + rotated.shape[0] - 1 >= height or dst_left < 0 or dst_left + rotated.shape[1] - 1 >= width:
                continue
            if stats is not None:
                stats['placed'] = stats.get('placed', 0) + 1
            window = score_map[dst_up:dst_up + rotated.shape[0], dst_left:dst_left + rotated.shape[1]]
            np.putmask(window, window < rotated, rotated)
            polygons.append(rotated_polygon(mat, polygon, nop) + (dst_left, dst_up))
    internal = case['internal']
    if internal is not None:
        box = seal['internal_box']
        value = internal['score'] if internal['score'] is not None else internal['mask']
        score_map[box[0]:box[0] + internal['height'], box[2]:box[2] + internal['width']] = value
        polygons.extend(internal_polygons(internal, box, (height, width)))
    with np.errstate(invalid='ignore', divide='ignore'):
        score_map = score_map * seal['alpha'] / score_map.max()
    return score_map.astype(np.float32), polygons


# ---- synthetic cases --------------------------------------------------------------------------------------------
def blocky(rng, shape, block, lo, hi, dtype):
    """a plane of ``block``-sized constant squares of integers in [lo, hi)"""
    h, w = shape
    coarse = rng.integers(lo, hi, (-(-h // block), -(-w // block)))
    return np.kron(coarse, np.ones((block, block), np.int64))[:h, :w].astype(dtype)


def make_glyph(rng, shape, kind):
    """(score float32 | None, image uint8): kind 'score' (score map + 1-channel image), 'gray' or 'lcd' (no score map)"""
    h, w = shape
    if kind == 'score':
        levels = blocky(rng, shape, 2, 0, 5, np.float32) / np.float32(4)
        levels[h // 2, w // 2] = 1.0
        return levels.astype(np.float32), (levels * 255).astype(np.uint8)
    if kind == 'gray':
        image = blocky(rng, shape, 2, 0, 3, np.uint8) * np.uint8(90)
        image[h // 2, w // 2] = 200
        return None, image
    image = np.stack([blocky(rng, shape, 2, 0, 2, np.uint8) * np.uint8(70 + 40 * c) for c in range(3)], axis=2)
    image[h // 2, w // 2, 1] = 9
    return None, image


def ring_slots(rng, shape, n, line_height, angles=None, reach=None):
    """``n`` char slots on a ring inside a seal of ``shape``: [angle, up_y, up_x, down_y, down_x]; the angle is the direction from
    down to up in whole degrees unless ``angles`` fixes it.  ``reach``: how far from the centre point_up lies (a fraction of the
    half extent)"""
    h, w = shape
    out = []
    for k in range(n):
        direction = (360.0 * k / n + float(rng.uniform(-3, 3))) % 360
        if angles is not None:
            direction = float(angles[k % len(angles)])
        theta = math.radians(direction)
        r = (0.42 if reach is None else reach)
        up_y = h / 2 + math.sin(theta) * r * h * 0.5
        up_x = w / 2 + math.cos(theta) * r * w * 0.5
        down_y = up_y - math.sin(theta) * line_height
        down_x = up_x - math.cos(theta) * line_height
        angle = round((math.atan2(up_y - down_y, up_x - down_x) % (2 * math.pi)) / (2 * math.pi) * 360)
        if angles is not None:
            angle = int(angles[k % len(angles)])
        out.append([angle, round(up_y, 3), round(up_x, 3), round(down_y, 3), round(down_x, 3)])
    return out


def make_line(rng, n_chars, height, interp, kinds=('score',), widths=(1, 15), match=None, resize_rows=None):
    """a horizontal text line of ``n_chars`` chars.  A char's box spans rows inside the line and columns next to one another; its
    glyph has the box's shape for the kinds without a score map (the mask way) and for the chars listed in ``match``, else its
    own (the resize).  ``resize_rows``: chars whose glyph differs from the box in BOTH dimensions."""
    chars, left = [], 0
    for k in range(n_chars):
        kind = kinds[k % len(kinds)]
        box_w = int(rng.integers(widths[0], widths[1]))
        up = int(rng.integers(0, 3))
        down = height - 1 - int(rng.integers(0, 3))
        box_h = down - up + 1
        shape = (box_h, box_w)
        if kind == 'score' and not (match and k in match):
            shape = (box_h + (int(rng.integers(1, 4)) if (resize_rows and k in resize_rows) else 0), box_w)
        score, image = make_glyph(rng, shape, kind)
        chars.append(dict(box=[up, down, left, left + box_w - 1], score=score, image=image, ref_h=height, ref_w=max(2, (height * 3) // 5)))
        left += box_w + 1
    return dict(height=height, width=max(left - 1, 1), interp=interp, chars=chars)


def make_internal(rng, box, with_score):
    h, w = box[1] - box[0] + 1, box[3] - box[2] + 1
    mask = (blocky(rng, (h, w), 2, 0, 2, np.uint8) > 0).astype(np.uint8)
    mask[h // 2, w // 2] = 1
    score = None
    if with_score:
        score = (blocky(rng, (h, w), 2, 0, 5, np.float32) / np.float32(4)).astype(np.float32)
    chars, left = [], 0
    while left + 3 <= w:
        chars.append(dict(box=[0, h - 1, left, left + 2], ref_h=h + 2, ref_w=4))
        left += 4
    return dict(height=h, width=w, score=score, mask=mask, chars=chars)


def make_case(seed, shape=(64, 64), n_chars=(5,), heights=(12,), interp='CUBIC', kinds=('score',), angles=None, internal=None,
              alpha=0.6, slots_per_line=None, indices=None, widths=(1, 15), reach=None, match=None, resize_rows=None, aspect=None):
    """one seal and its text lines.  ``n_chars`` / ``heights``: per text line; ``slots_per_line``: char slots per text-line slot
    (default: as many as chars); ``indices``: the text-line slot indices (default 0, 1, ...); ``internal``: None, 'score' or
    'mask'"""
    rng = np.random.default_rng(seed)
    h, w = shape
    slots, lines = [], []
    for k, (n, height) in enumerate(zip(n_chars, heights)):
        n_slots = n if slots_per_line is None else slots_per_line[k]
        slots.append(dict(height=height, aspect=float(aspect if aspect is not None else round(float(rng.uniform(0.4, 0.9)), 3)),
                          chars=ring_slots(rng, shape, n_slots, height, angles, reach)))
        lines.append(make_line(rng, n, height, INTERPOLATIONS[interp], kinds, widths, match, resize_rows))
    internal_box = internal_line = None
    if internal:
        ih, iw = max(3, h // 6), max(6, w // 2)
        internal_box = [h // 2 - 1, h // 2 - 1 + ih - 1, (w - iw) // 2, (w - iw) // 2 + iw - 1]
        internal_line = make_internal(rng, internal_box, internal == 'score')
    return dict(seal=dict(h=h, w=w, alpha=alpha, slots=slots, internal_box=internal_box),
                indices=list(range(len(lines))) if indices is None else list(indices), lines=lines, internal=internal_line)


# The cases of tests/golden/seal_impression.npz and of tests/test_gpu_seal_impression.py: name -> make_case arguments.
BRANCH_ANGLES = (270 + 0, 270 + 37, 270 + 90, 270 + 135, 270 + 180, 270 + 200, 270 - 270, 270 + 300, 270 + 269)
CASES = {
    'one_char': dict(seed=1, shape=(48, 64), n_chars=(1,), heights=(9,), interp='CUBIC'),
    'five_cubic': dict(seed=2, shape=(64, 64), n_chars=(5,), heights=(12,), interp='CUBIC', resize_rows=(1, 3)),
    'five_lanczos': dict(seed=3, shape=(97, 61), n_chars=(5,), heights=(16,), interp='LANCZOS4', resize_rows=(0, 2)),
    'five_linear': dict(seed=4, shape=(64, 64), n_chars=(5,), heights=(11,), interp='LINEAR_EXACT', resize_rows=(4,)),
    'five_nearest': dict(seed=5, shape=(48, 64), n_chars=(5,), heights=(10,), interp='NEAREST_EXACT', resize_rows=(2,)),
    'five_area': dict(seed=6, shape=(64, 64), n_chars=(5,), heights=(13,), interp='AREA', aspect=0.2, widths=(8, 15), resize_rows=(1, 2)),
    'branches': dict(seed=7, shape=(97, 61), n_chars=(9,), heights=(10,), interp='CUBIC', angles=BRANCH_ANGLES, reach=0.35),
    'overlap': dict(seed=8, shape=(64, 64), n_chars=(12,), heights=(14,), interp='CUBIC', reach=0.2, aspect=0.9, widths=(10, 15)),
    'width_one': dict(seed=9, shape=(48, 64), n_chars=(5,), heights=(9,), interp='CUBIC', widths=(1, 3), aspect=0.1),
    'copied': dict(seed=10, shape=(64, 64), n_chars=(5,), heights=(12,), interp='CUBIC', match=(0, 1, 2, 3, 4), aspect=0.6),
    'mask_way': dict(seed=11, shape=(64, 64), n_chars=(6,), heights=(12,), interp='CUBIC', kinds=('lcd', 'gray'), aspect=0.6),
    'out_of_bound': dict(seed=12, shape=(48, 64), n_chars=(8,), heights=(14,), interp='CUBIC', reach=1.0),
    'more_chars_than_slots': dict(seed=13, shape=(64, 64), n_chars=(7,), heights=(11,), interp='CUBIC', slots_per_line=(4,)),
    'slot_index_out_of_range': dict(seed=14, shape=(64, 64), n_chars=(4, 4), heights=(10, 12), interp='CUBIC', indices=(0, 5)),
    'internal_score': dict(seed=15, shape=(64, 64), n_chars=(10,), heights=(12,), interp='CUBIC', internal='score', reach=0.15),
    'internal_mask': dict(seed=16, shape=(97, 61), n_chars=(10,), heights=(12,), interp='LANCZOS4', internal='mask', reach=0.15),
    'all_zero': dict(seed=17, shape=(48, 64), n_chars=(3,), heights=(9,), interp='CUBIC', reach=1.5),
    'two_lines_60': dict(seed=18, shape=(97, 61), n_chars=(30, 30), heights=(9, 10), interp='CUBIC', widths=(1, 8), reach=0.4),
}
# The mask way with a resize: the reference stops at an assert there (Mask.to_resized_mask on a box-attached mask), so these have no
# golden; the restatement is what `python -O` would make the reference compute.
MASK_RESIZE_CASES = {
    'mask_' + interp.lower(): dict(seed=30 + k, shape=(64, 64), n_chars=(6,), heights=(12,), interp=interp, kinds=('lcd', 'gray'),
                                   aspect=(0.25 if interp == 'AREA' else 0.8), widths=(6, 15))
    for k, interp in enumerate(INTERPOLATIONS)
}


def case(name):
    return make_case(**(CASES[name] if name in CASES else MASK_RESIZE_CASES[name]))


# ---- tests/golden/seal_impression.npz and .json ---------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'seal_impression')
_golden = {}


def golden():
    """(index, get): the JSON index kept in the .npz and the reader of its [offset, shape, dtype] array references"""
    if not _golden:
        _golden['arrays'] = dict(np.load(GOLDEN + '.npz'))
        _golden['index'] = json.loads(str(_golden['arrays']['index']))

    def get(ref):
        if ref is None:
            return None
        at, shape, dtype = ref
        return _golden['arrays'][dtype][at:at + int(np.prod(shape))].reshape(shape)
    return _golden['index'], get


def golden_case(row, get):
    """the case a ``fills`` row of the golden index holds"""
    def chars(line):
        return [dict(box=c['box'], score=get(c['score']), image=get(c['image']), ref_h=c['ref_h'], ref_w=c['ref_w']) for c in line['chars']]
    internal = row['internal']
    return dict(seal=row['seal'], indices=row['indices'],
                lines=[dict(height=line['height'], width=line['width'], interp=line['interp'], chars=chars(line)) for line in row['lines']],
                internal=None if internal is None else dict(height=internal['height'], width=internal['width'], score=get(internal['score']),
                                                            mask=get(internal['mask']), chars=chars(internal)))


def same_bits(a, b):
    """two float32 arrays agree bit for bit, a NaN on one side being a NaN on the other"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool((nan_a == nan_b).all()) and a[~nan_a].tobytes() == b[~nan_b].tobytes()


# ---- a plain-data case as the package's objects (imported on use: the restatement itself needs neither package nor library) ----
def amd_items(case, device=False):
    """(seal_impression, text_line_slot_indices, text_lines, internal_text_line) of a case; ``device``: glyph planes and the
    internal line's planes are device-resident"""
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Image, Mask, Point, ScoreMap
    from vkit_amd.engine.font import CharBox, CharGlyph, TextLine
    from vkit_amd.engine.seal_impression import CharSlot, SealImpression, TextLineSlot
    ctx = N.default_ctx()
    put = (lambda a: ctx.to_device(np.ascontiguousarray(a))) if device else (lambda a: a)
    seal = case['seal']
    slots = [TextLineSlot(text_line_height=s['height'], char_aspect_ratio=s['aspect'],
                          char_slots=[CharSlot(angle=c[0], point_up=Point.create(y=c[1], x=c[2]), point_down=Point.create(y=c[3], x=c[4]))
                                      for c in s['chars']]) for s in seal['slots']]
    box = seal['internal_box']
    seal_impression = SealImpression(alpha=seal['alpha'], color=(200, 0, 0), background_mask=Mask(mat=np.zeros((seal['h'], seal['w']), np.uint8)),
                                     text_line_slots=slots,
                                     internal_text_line_box=None if box is None else Box(up=box[0], down=box[1], left=box[2], right=box[3]))

    def line_of(line, internal=False):
        h, w = line['height'], line['width']
        line_box = Box(up=0, down=h - 1, left=0, right=w - 1)
        char_boxes = [CharBox(char='x', box=Box(up=c['box'][0], down=c['box'][1], left=c['box'][2], right=c['box'][3])) for c in line['chars']]
        if internal:
            glyphs = [CharGlyph(image=Image(mat=np.zeros((c['box'][1] - c['box'][0] + 1, 3), np.uint8)), score_map=None,
                                ref_char_height=c['ref_h'], ref_char_width=c['ref_w']) for c in line['chars']]
            mask = Mask(mat=put(line['mask']), box=line_box)
            score_map = None if line['score'] is None else ScoreMap(mat=put(line['score']), box=line_box)
        else:
            glyphs = [CharGlyph(image=Image(mat=put(c['image'])), score_map=None if c['score'] is None else ScoreMap(mat=put(c['score'])),
                                ref_char_height=c['ref_h'], ref_char_width=c['ref_w']) for c in line['chars']]
            mask, score_map = Mask(mat=np.ones((h, w), np.uint8), box=line_box), None
        return TextLine(image=Image(mat=np.zeros((h, w, 3), np.uint8), box=line_box), mask=mask, score_map=score_map, char_boxes=char_boxes,
                        char_glyphs=glyphs, cv_resize_interpolation=line.get('interp', 2), is_hori=True)

    internal = case['internal']
    return (seal_impression, case['indices'], [line_of(line) for line in case['lines']],
            None if internal is None else line_of(internal, internal=True))
