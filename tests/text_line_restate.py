"""numpy-plus-oracle restatement of the pixel half of render_text_line_meta (reference: engine/font/freetype.py:314-380 the paste,
:600-837 resize, pad, trim and the clean-up of a trimmed char) for the tests of csrc/text_line.hip and of
vkit_amd.engine.font.text_line, a deterministic fake glyph rasteriser, and the cases those tests and
tests/golden/make_text_line_golden.py share.  Tests only: the product never imports this.

``render_pixels`` takes what the placement left -- the trimmed glyph arrays, their boxes in the pasted plane and its shape -- and
the run config's numbers, and does on whole arrays what the reference does: paste, oracle.resize of the three planes, pad, trim
and clean-up, with the decisions those steps hang on.  It returns ``None`` where the reference cannot trim and raises numpy's
``ValueError`` where the reference writes into a read-only score map.

The fake rasteriser (``fake_glyph``) makes blocky synthetic bitmaps keyed by char and nominal size, in three kinds: 'default'
(2-D, 0..255), 'lcd' (3-D) and 'mono' (0 / 255).  ``bitmap_top``, ``bitmap_left`` (negative for some chars) and ``advance.x``
(with half pixels) vary with the char; some bitmaps have empty border rows and columns so that the trimmers of build_char_glyph
act.  '.' is a 1 x 1 glyph; 'L' and 'T' are the letters' shapes, which kern into one another; 'H' is a full block without pads.
"""
import json
import os
from types import SimpleNamespace

import numpy as np

import oracle as O

INTERPOLATIONS = dict(NEAREST_EXACT=6, LINEAR_EXACT=5, CUBIC=2, LANCZOS4=4, AREA=3)
CHARS = 'abcdefghijklmnopqrstuvwxyzHLT.'


# ---- the fake rasteriser ------------------------------------------------------------------------------------------
def blocky(rng, shape, block, lo, hi):
    h, w = shape
    coarse = rng.integers(lo, hi, (-(-h // block), -(-w // block)))
    return np.kron(coarse, np.ones((block, block), np.int64))[:h, :w]


def fake_glyph(char, kind, size):
    """(glyph slot, bitmap) of ``char``: the slot has ``bitmap_top``, ``bitmap_left`` and ``advance.x`` / ``.y`` in 1/64 pixel"""
    code = ord(char)
    rng = np.random.default_rng([code, size, 7])
    levels = {'default': 4, 'lcd': 4, 'mono': 2}[kind]
    unit = {'default': 85, 'lcd': 85, 'mono': 255}[kind]
    top_cut, left = code % 3, code % 4 - 1
    if char == '.':
        plane = np.full((1, 1), levels - 1, np.int64)
        top, left, advance = 1, 0, 3 * 64
    elif char == 'H':
        h, w = size, max(1, size // 2)
        plane = 1 + blocky(rng, (h, w), 2, 0, levels - 1)
        top, left, advance = h, 0, w * 64
    elif char in 'LT':
        h, w = size, max(3, (size * 2) // 3)
        plane = np.zeros((h, w), np.int64)
        if char == 'L':
            plane[:, 0] = levels - 1
            plane[h - 1, :] = 1
        else:
            plane[0, :] = levels - 1
            plane[:, w // 2] = 1
        top, left, advance = h, 0, w * 64
    else:
        h, w = max(1, size - top_cut), max(1, (size * (3 + code % 4)) // 6)
        plane = blocky(rng, (h, w), 2, 0, levels)
        plane[h // 2, w // 2] = levels - 1
        if code % 5 == 0:                       # empty border rows and columns: the trimmers act
            plane = np.pad(plane, ((1, code % 2), (1, 2)))
        top = plane.shape[0] - top_cut
        advance = 64 * (plane.shape[1] + code % 3 + max(0, left)) + 32 * (code % 2)
    bitmap = (plane * unit).astype(np.uint8)
    if kind == 'lcd':                           # the channels differ; ink stays where the plane has it
        shade = rng.integers(0, 3, plane.shape + (3,))
        bitmap = (np.clip(plane[:, :, None] - shade, 0, levels - 1) * unit).astype(np.uint8)
        bitmap[plane > 0, code % 3] = np.maximum(bitmap[plane > 0, code % 3], 40)
    slot = SimpleNamespace(bitmap_top=int(top), bitmap_left=int(left), advance=SimpleNamespace(x=int(advance), y=0))
    return slot, bitmap


def make_renderer(kind, size, build_char_glyph):
    """``func_render_char_glyph`` for render_text_line_meta, through the given ``build_char_glyph`` (the reference's or the package's)"""
    def render(run_config, font_face, char):
        slot, bitmap = fake_glyph(char, kind, size)
        return build_char_glyph(run_config, char, slot, bitmap)
    return render


FONT_INFO = dict(tags=['all'], ascent_plus_pad_up_min_to_font_size_ratio=0.7, height_min_to_font_size_ratio=0.9,
                 width_min_to_font_size_ratio=0.5)


def run_config_of(case, types):
    """the FontEngineRunConfig of a case, built from the classes of ``types`` (the reference's font type module or the package's)"""
    collection = types.FontGlyphInfoCollection(font_glyph_infos=[types.FontGlyphInfo(**FONT_INFO)])
    variant = types.FontVariant(char_to_tags={c: ['all'] for c in CHARS}, font_file='fake.ttf', font_glyph_info_collection=collection)
    style = dict(font_size_ratio=case['size'] / (case['height'] if case['hori'] else case['width']), font_size_min=1)
    style.update(case['style'])
    if 'glyph_color' in style:
        style['glyph_color'] = tuple(style['glyph_color'])
    sequence = types.FontEngineRunConfigGlyphSequence.HORI_DEFAULT if case['hori'] else types.FontEngineRunConfigGlyphSequence.VERT_DEFAULT
    return types.FontEngineRunConfig(height=case['height'], width=case['width'], chars=list(case['text']), font_variant=variant,
                                     glyph_sequence=sequence, style=types.FontEngineRunConfigStyle(**style))


# ---- the cases ----------------------------------------------------------------------------------------------------
TIGHT = dict(prob_set_char_space_min=1.0)       # every char space is round(char_space_min) = 0


def _case(text, height, width, size, kind='default', hori=True, enlarge='CUBIC', shrink='AREA', seed=0, expect='line', **style):
    return dict(text=text, height=height, width=width, size=size, kind=kind, hori=hori, enlarge=INTERPOLATIONS[enlarge],
                shrink=INTERPOLATIONS[shrink], seed=seed, expect=expect, style=style)


# expect: 'line', 'none' (cannot trim) or 'value_error'; what each case is named for is asserted by tests/test_text_line_golden.py
CASES = {
    # horizontal, default glyphs
    'one_char': _case('g', 14, 40, 12),
    'one_pixel_glyph': _case('.', 12, 16, 12),
    'kerning_overlap': _case('LTLT', 14, 60, 12, **TIGHT),
    'words': _case('ab cd  efg', 16, 160, 13, glyph_color=(10, 200, 30)),
    'enlarge_nearest': _case('abcd', 24, 160, 8, enlarge='NEAREST_EXACT'),
    'enlarge_linear': _case('bcde', 25, 160, 9, enlarge='LINEAR_EXACT'),
    'enlarge_cubic': _case('cdef', 27, 160, 8, enlarge='CUBIC'),
    'enlarge_lanczos': _case('defg', 23, 160, 7, enlarge='LANCZOS4'),
    'shrink_nearest': _case('efgh', 13, 160, 22, shrink='NEAREST_EXACT'),
    'shrink_linear': _case('fghi', 14, 160, 23, shrink='LINEAR_EXACT'),
    'shrink_cubic': _case('ghij', 12, 160, 21, shrink='CUBIC'),
    'shrink_lanczos': _case('hijk', 15, 160, 24, shrink='LANCZOS4'),
    'shrink_area_integer': _case('HHHH', 12, 160, 24, shrink='AREA', **TIGHT),
    'shrink_area_fraction': _case('ijkl', 15, 160, 22, shrink='AREA'),
    'shrink_linear_half': _case('HHH', 13, 160, 26, shrink='LINEAR_EXACT', **TIGHT),
    'pad_even': _case('HHHH', 18, 160, 16, **TIGHT),
    'pad_odd': _case('HHHH', 19, 160, 16, **TIGHT),
    'trim_no_overlap': _case('abcdefgh', 14, 40, 12),
    'trim_cleanup': _case('HLTH', 14, 16, 12, **TIGHT),
    'trim_cleanup_resized': _case('HLTH', 20, 28, 12, enlarge='CUBIC', **TIGHT),
    'trim_cleanup_shrunk': _case('HLTH', 12, 16, 20, shrink='AREA', **TIGHT),
    'trim_cleanup_linear': _case('HLTH', 21, 29, 12, enlarge='LINEAR_EXACT', **TIGHT),
    'trim_drop_last': _case('aq', 24, 35, 12, enlarge='CUBIC'),
    'untrimmable': _case('HHHH', 36, 16, 36, expect='none', **TIGHT),
    # LCD
    'lcd_gamma_1': _case('abc de', 16, 160, 13, kind='lcd'),
    'lcd_gamma_2.2': _case('bcd ef', 16, 160, 13, kind='lcd', glyph_color_gamma=2.2),
    'lcd_kerning': _case('LTLT', 14, 60, 12, kind='lcd', **TIGHT),
    'lcd_enlarge_cleanup': _case('HLTH', 20, 28, 12, kind='lcd', enlarge='LANCZOS4', glyph_color_gamma=1.8, **TIGHT),
    'default_gamma': _case('cde fg', 16, 160, 13, glyph_color_gamma=2.2, glyph_color=(200, 0, 90)),
    # monochrome
    'mono_enlarge': _case('abcd', 24, 160, 8, kind='mono', enlarge='NEAREST_EXACT', shrink='NEAREST_EXACT'),
    'mono_shrink': _case('efgh', 13, 160, 22, kind='mono', enlarge='NEAREST_EXACT', shrink='NEAREST_EXACT'),
    # vertical
    'vert_resized': _case('abcd', 120, 24, 8, hori=False, enlarge='CUBIC'),
    'vert_shrunk': _case('efg', 120, 12, 22, hori=False, shrink='AREA'),
    'vert_padded_lcd': _case('HHH', 120, 14, 24, hori=False, kind='lcd'),
    'vert_padded_default': _case('HHH', 120, 14, 24, hori=False, expect='value_error'),
    'vert_trimmed': _case('abcdefgh', 40, 16, 12, hori=False, enlarge='LINEAR_EXACT', shrink='LINEAR_EXACT'),
    'vert_untrimmable': _case('HH', 16, 12, 24, hori=False, expect='none'),
}


def case(name):
    return dict(CASES[name], name=name)


def random_cases(count=30, seed=20241019):
    """small random lines for the batch test: (name, case)"""
    rng = np.random.default_rng(seed)
    letters = [c for c in CHARS if c != '.']
    codes = sorted(INTERPOLATIONS)
    out = []
    for k in range(count):
        n = int(rng.integers(1, 9))
        text = ''.join(letters[int(i)] for i in rng.integers(0, len(letters), n))
        if n > 3 and k % 3 == 0:
            text = text[:2] + ' ' + text[2:]
        hori = bool(k % 5)
        kind = ('default', 'lcd', 'mono')[k % 3]
        if not hori and kind != 'lcd':
            kind = 'lcd' if k % 2 else kind     # (a padded vertical default line is the reference's ValueError)
        enlarge = [c for c in codes if c != 'AREA'][int(rng.integers(0, 4))]
        shrink = codes[int(rng.integers(0, 5))]
        size = int(rng.integers(6, 26))
        target, other = int(rng.integers(12, 33)), int(rng.integers(16, 120))
        out.append((f'random_{k}', _case(text, target if hori else other, other if hori else target, size, kind=kind, hori=hori,
                                         enlarge=enlarge, shrink=shrink, seed=100 + k)))
    return out


# ---- the pixel half -----------------------------------------------------------------------------------------------
def glyph_mask(image):
    return ((image > 0) if image.ndim == 2 else np.any(image > 0, axis=2)).astype(np.uint8)


def resized_image(image, shape, interp):
    return O.resize(image, shape, interp)


def resized_mask(mask, shape, interp):
    return (O.resize(mask * np.uint8(255), shape, interp) > 0).astype(np.uint8)


def resized_score(score, shape, interp):
    return np.clip(O.resize(score, shape, interp), 0.0, 1.0).astype(np.float32)


def conducted(box, shape, resized):
    def one(value, size, resized_size):
        return round(max(0, min(value * resized_size / size, resized_size - 1)))
    up, down, left, right = box
    return [one(up, shape[0], resized[0]), one(down, shape[0], resized[0]), one(left, shape[1], resized[1]), one(right, shape[1], resized[1])]


def paste(glyphs, boxes, shape, color, gamma):
    """reference :314-380: (image, mask, score | None)"""
    height, width = shape
    image = np.full((height, width, 3), 255, np.uint8)
    mask = np.zeros((height, width), np.uint8)
    lcd = glyphs[0]['image'].ndim == 3
    score = None if lcd else np.zeros((height, width), np.float32)
    for glyph, (up, down, left, right) in zip(glyphs, boxes):
        ink = glyph_mask(glyph['image']).astype(bool)
        assert ink.shape == (down - up + 1, right - left + 1)
        if lcd:
            value = ((1 - np.power(glyph['image'] / 255.0, gamma)) * 255).astype(np.uint8)
        else:
            value = np.empty(ink.shape + (3,), np.uint8)      # (RGBA with the score map as alpha; RGBA2RGB drops the alpha)
            value[:] = color
        image[up:down + 1, left:right + 1][ink] = value[ink]
        mask[up:down + 1, left:right + 1][ink] = 1
        if not lcd:
            window = score[up:down + 1, left:right + 1]
            np.putmask(window, window < glyph['score'], glyph['score'])
    return image, mask, score


def render_pixels(glyphs, boxes, shape, case):
    """-> None | dict(image, mask, score | None, boxes, interp).  ``glyphs``: [{image uint8, score float32 | None}] as
    build_char_glyph left them; ``boxes``: [[up, down, left, right]] in the pasted plane of ``shape``"""
    style = dict(glyph_color=(0, 0, 0), glyph_color_gamma=1.0)
    style.update(case['style'])
    image, mask, score = paste(glyphs, boxes, shape, tuple(style['glyph_color']), style['glyph_color_gamma'])
    hori = case['hori']
    target = case['height'] if hori else case['width']
    own = image.shape[0] if hori else image.shape[1]
    too_small, too_large = own / target < 0.8, own > target
    interp = case['shrink'] if too_large else case['enlarge']
    boxes = [list(b) for b in boxes]
    if too_small or too_large:
        h, w = image.shape[:2]
        resized = (target, round(target * w / h)) if hori else (round(target * h / w), target)
        boxes = [conducted(b, (h, w), resized) for b in boxes]
        image, mask = resized_image(image, resized, interp), resized_mask(mask, resized, interp)
        if score is not None:
            score = resized_score(score, resized, interp)
    h, w = image.shape[:2]
    if hori and h != target:
        pad = target - h
        assert pad > 0
        before, after = pad // 2, pad - pad // 2
        image = np.concatenate([np.full((before, w, 3), 255, np.uint8), image, np.full((after, w, 3), 255, np.uint8)])
        mask = np.concatenate([np.zeros((before, w), np.uint8), mask, np.zeros((after, w), np.uint8)])
        if score is not None:
            score = np.concatenate([np.zeros((before, w), np.float32), score, np.zeros((after, w), np.float32)])
        boxes = [[b[0] + before, b[1] + before, b[2], b[3]] for b in boxes]
    if not hori and w != target:
        pad = target - w
        assert pad > 0
        before, after = pad // 2, pad - pad // 2
        image = np.concatenate([np.full((h, before, 3), 255, np.uint8), image, np.full((h, after, 3), 255, np.uint8)], axis=1)
        mask = np.concatenate([np.zeros((h, before), np.uint8), mask, np.zeros((h, after), np.uint8)], axis=1)
        boxes = [[b[0], b[1], b[2] + before, b[3] + after] for b in boxes]      # (left by the left pad, right by the right pad)
        if score is not None:
            raise ValueError('assignment destination is read-only')
    h, w = image.shape[:2]
    limit = case['width'] if hori else case['height']
    far = 3 if hori else 1                      # a box's right or down
    if (w if hori else h) > limit:
        last = len(boxes) - 1
        while last >= 0 and boxes[last][far] >= limit:
            last -= 1
        if last == len(boxes) - 1:
            last -= 1
        if last < 0 or boxes[last][far] >= limit:
            return None
        end = boxes[last][far]
        if hori and boxes[last + 1][2] <= end:
            # the residual pixels of the first trimmed char
            image, mask = image.copy(), mask.copy()
            up, down, left, right = boxes[last + 1]
            trimmed = glyph_mask(glyphs[last + 1]['image'])
            if trimmed.shape != (down - up + 1, right - left + 1):
                trimmed = resized_mask(trimmed, (down - up + 1, right - left + 1), interp)
            image[up:down + 1, left:right + 1][trimmed > 0] = 255
            mask[up:down + 1, left:right + 1][trimmed > 0] = 0
            if score is not None:
                score = score.copy()
                score[up:down + 1, left:right + 1] = 0
                up, down, left, right = boxes[last]
                kept = glyphs[last]['score']
                if kept.shape != (down - up + 1, right - left + 1):
                    kept = resized_score(kept, (down - up + 1, right - left + 1), interp)
                window = score[up:down + 1, left:right + 1]
                np.putmask(window, window < kept, kept)
        boxes = boxes[:last + 1]
        image = image[:, :end + 1] if hori else image[:end + 1]
        mask = mask[:, :end + 1] if hori else mask[:end + 1]
        if score is not None:
            score = score[:, :end + 1] if hori else score[:end + 1]
    return dict(image=np.ascontiguousarray(image), mask=np.ascontiguousarray(mask), score=None if score is None else np.ascontiguousarray(score),
                boxes=boxes, interp=interp)


# ---- tests/golden/text_line.npz and .json -------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'text_line')
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


def golden_glyphs(row, get):
    return [dict(image=get(g['image']), score=get(g['score'])) for g in row['glyphs']]


def same_bits(a, b):
    """two arrays agree in shape, dtype and bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- a case through the package (imported on use: the restatement itself needs neither package nor library) ----------------
def amd_arguments(case):
    """(run_config, font_face, func_render_char_glyph, enlarge, shrink) of a case for the package's render_text_line_meta / TextLineBatch.add"""
    from vkit_amd.engine.font import text_line as TL, type as FT
    return run_config_of(case, FT), None, make_renderer(case['kind'], case['size'], TL.build_char_glyph), case['enlarge'], case['shrink']


def box_list(char_boxes):
    return [[b.up, b.down, b.left, b.right] for b in char_boxes]
