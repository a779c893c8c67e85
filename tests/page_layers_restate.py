"""The page's symbol, barcode and frame layers restated in numpy on the oracle's cv.resize -- what csrc/page_layers.hip computes
(vkx_page_layers_dev) and what the reference's steps compute (pipeline/text_detection/page_non_text_symbol.py:107-169,
engine/barcode/qr.py:81-93 and code39.py:137-148, page_text_line_bounding_box.py:94-147) -- together with the synthetic inputs of
tests/golden/make_page_layers_golden.py: the symbol textures, the module generators that stand in for the two third-party
barcode encoders, the frame layouts, and the loader of tests/golden/page_layers.npz.

Every float32 operation is one numpy operation on float32 operands, so each is rounded once, as on the device."""
import json
import os
from types import SimpleNamespace

import numpy as np

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
CUBIC = 2


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def symbol_rgba(src, out_shape, alpha):
    """-> (image uint8 (oh, ow, 3), alpha plane float32 (oh, ow)); an all-zero alpha channel gives NaN throughout (0 / 0)."""
    resized = O.resize(np.ascontiguousarray(src), out_shape, CUBIC)
    a = resized[:, :, 3]
    with np.errstate(invalid='ignore', divide='ignore'):
        plane = ((a.astype(F32) / F32(255)) * F32(alpha)) / (F32(a.max()) / F32(255))
    return np.ascontiguousarray(resized[:, :, :3]), plane.astype(F32)


def symbol_gray(src, out_shape, alpha, color):
    g = O.resize(np.ascontiguousarray(src), out_shape, CUBIC)
    image = np.empty(tuple(out_shape) + (3,), np.uint8)
    image[:] = np.array(color, np.uint8)
    return image, np.where(g > 0, F32(alpha), F32(0)).astype(F32)


def score(mask, out_shape, alpha):
    """-> (plane, the resize before its clip or None when nothing is resized)"""
    s = np.where(np.asarray(mask) > 0, F32(alpha), F32(0)).astype(F32)
    if s.shape == tuple(out_shape):
        return s, None
    raw = O.resize(s, out_shape, CUBIC)
    return np.clip(raw, 0.0, 1.0).astype(F32), raw


def frame(box_shape, thickness, alpha, trims):
    box_h, box_w = box_shape
    plane = np.full((box_h, box_w), F32(alpha), F32)
    plane[thickness:box_h - thickness, thickness:box_w - thickness] = 0
    up, down, left, right = trims
    return np.ascontiguousarray(plane[up:box_h - down, left:box_w - right])


def same_bits(got, want):
    """uint8 exactly; float32 under ``==`` with equal NaN positions"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != 'f':
        return bool((got == want).all())
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got[~nan] == want[~nan]).all())


# ---- synthetic inputs ----------------------------------------------------------------------------------------------------------
def blocky(rng, shape, block, lo, hi):
    small = rng.integers(lo, hi, size=((shape[0] + block - 1) // block, (shape[1] + block - 1) // block))
    return np.ascontiguousarray(np.kron(small, np.ones((block, block), np.int64))[:shape[0], :shape[1]].astype(np.uint8))


def _rgba(rng, shape, alpha_plane):
    tex = rng.integers(0, 256, size=shape + (4,)).astype(np.uint8)
    tex[:, :, 3] = alpha_plane
    return tex


def symbol_textures():
    """name -> uint8 texture ((h, w, 4) RGBA or (h, w) grayscale); the file list of the fake selector is the sorted names"""
    rng = np.random.default_rng(20241105)
    tex = {}
    tex['rgba_9x7'] = _rgba(rng, (9, 7), rng.integers(0, 256, size=(9, 7)))
    tex['rgba_24x30'] = _rgba(rng, (24, 30), blocky(rng, (24, 30), 5, 0, 200))
    tex['rgba_12x12'] = _rgba(rng, (12, 12), rng.integers(1, 256, size=(12, 12)))
    tex['rgba_8x8'] = _rgba(rng, (8, 8), rng.integers(0, 120, size=(8, 8)))
    tex['rgba_6x6'] = _rgba(rng, (6, 6), rng.integers(0, 256, size=(6, 6)))
    tex['rgba_zero'] = _rgba(rng, (10, 10), 0)
    peak = rng.integers(0, 41, size=(10, 70)).astype(np.uint8)
    peak[9, 69] = 255                       # the maximum on one pixel, in the last (partial) 64 x 4 tile of the plane
    tex['rgba_peak'] = _rgba(rng, (10, 70), peak)
    tex['gray_7x9'] = blocky(rng, (7, 9), 2, 0, 3) * np.uint8(90)
    sparse = np.zeros((40, 40), np.uint8)   # sparse ink: the cubic undershoot saturates to 0 next to values > 0
    sparse[rng.integers(0, 40, 30), rng.integers(0, 40, 30)] = 255
    sparse[10:14, 20:31] = 200
    tex['gray_sparse'] = sparse
    tex['gray_zero'] = np.zeros((11, 13), np.uint8)
    tex['rgb_3ch'] = rng.integers(0, 256, size=(5, 5, 3)).astype(np.uint8)
    return tex


# (texture, (out_h, out_w), layout alpha)
RGBA_CASES = [('rgba_9x7', (13, 11), 0.8), ('rgba_24x30', (17, 13), 0.55), ('rgba_12x12', (12, 12), 1.0), ('rgba_8x8', (5, 131), 0.7),
              ('rgba_6x6', (1, 1), 0.9), ('rgba_zero', (14, 9), 0.6), ('rgba_peak', (10, 70), 0.75)]
GRAY_CASES = [('gray_7x9', (20, 33), 0.85), ('gray_sparse', (9, 9), 0.5), ('gray_zero', (6, 17), 0.95), ('gray_7x9', (7, 9), 0.3)]
FILES = sorted(symbol_textures())
SYMBOL_PAGES = 12                           # seeded pages of a few symbols each, drawn over FILES without the 3-channel file


def symbol_page_layout(seed):
    """the symbol boxes and alphas of seeded page ``seed``: [(up, left, h, w, alpha)] on a 160 x 200 page"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(int(rng.integers(2, 6))):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 140))
        out.append((int(rng.integers(0, 160 - h + 1)), int(rng.integers(0, 200 - w + 1)), h, w, float(rng.uniform(0.3, 1.0))))
    return out


def _text_bits(text, n):
    rng = np.random.default_rng([ord(c) for c in text] + [n])
    return rng


def qr_image(text):
    """A 25 x 25 module image in the encoder's convention (255 background, 0 ink): finder squares and text-seeded modules."""
    rng = _text_bits(text, 25)
    ink = rng.random((25, 25)) < 0.5
    for y, x in ((0, 0), (0, 18), (18, 0)):
        ink[y:y + 7, x:x + 7] = True
        ink[y + 1:y + 6, x + 1:x + 6] = False
        ink[y + 2:y + 5, x + 2:x + 5] = True
    return np.where(ink, 0, 255).astype(np.uint8)


def code39_image(text):
    """A 40 x 150 strip with a quiet zone (the trim of convert_barcode_pil_image_to_mask runs): text-seeded bars."""
    rng = _text_bits(text, 39)
    image = np.full((40, 150), 255, np.uint8)
    x = 10
    while x < 138:
        bar, gap = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        image[4:36, x:min(x + bar, 138)] = 0
        x += bar + gap
    image[4:36, 137] = 0
    return image


# (engine, init overrides, (height, width), seed)
BARCODE_CASES = [('qr', {}, (64, 64), 0), ('qr', {}, (25, 25), 1), ('qr', {}, (23, 23), 2), ('code39', {}, (20, 131), 3),
                 ('qr', dict(alpha_min=1.0, alpha_max=1.0), (64, 64), 4), ('code39', dict(alpha_min=1.0, alpha_max=1.0), (32, 106), 5)]
# a page of barcode boxes (up, left, h, w): two QR codes and one code-39
BARCODE_PAGE = dict(shape=(200, 240), qrs=[(5, 5, 64, 64), (100, 20, 25, 25)], code39s=[(150, 60, 20, 131)], seed=11)

# single frames: name -> (page h, page w, text-line box (up, down, left, right), ref_char_height, config overrides); the seed of each is
# searched by the golden maker so that the named trims (and nothing else) occur
FRAME_CASES = {
    'no_trim': (200, 300, (80, 99, 100, 199), 20, {}, ()),
    'trim_up': (200, 300, (2, 21, 100, 199), 20, {}, ('up',)),
    'trim_down': (200, 300, (178, 197, 100, 199), 20, {}, ('down',)),
    'trim_left': (200, 300, (80, 99, 2, 101), 20, {}, ('left',)),
    'trim_right': (200, 300, (80, 99, 198, 297), 20, {}, ('right',)),
    'trim_all': (60, 100, (20, 39, 10, 89), 20, {}, ('up', 'down', 'left', 'right')),
    'thin': (200, 300, (80, 99, 100, 199), 20, dict(border_thickness_ratio_max=0.0), ()),
}
FRAME_RUN_SEEDS = tuple(range(8))


def frame_run_lines(seed):
    """the text lines of seeded frame page ``seed`` (160 x 220): [(box (up, down, left, right), [ref_char_height], colour, short)]"""
    rng = np.random.default_rng(2000 + seed)
    lines = []
    for k in range(12):
        h, w = int(rng.integers(8, 24)), int(rng.integers(20, 120))
        up, left = int(rng.integers(0, 160 - h + 1)), int(rng.integers(0, 220 - w + 1))
        lines.append(((up, up + h - 1, left, left + w - 1), [h, max(4, h - 3)], tuple(int(v) for v in rng.integers(0, 256, 3)), bool(k % 2)))
    return lines


FRAME_RUN_CONFIG = dict(prob_non_short_text_line=0.5, prob_short_text_line=0.8)


def text_line_of(box, ref_heights, color, box_cls):
    up, down, left, right = box
    return SimpleNamespace(box=box_cls(up=up, down=down, left=left, right=right), glyph_color=tuple(color),
                           char_glyphs=[SimpleNamespace(ref_char_height=h) for h in ref_heights])


# ---- the golden file -----------------------------------------------------------------------------------------------------------
def golden():
    """(index, get): the JSON index of tests/golden/page_layers.npz and ``get(entry)`` -> the array an index entry names"""
    data = np.load(os.path.join(HERE, 'golden', 'page_layers.npz'))
    index = json.loads(str(data['index']))

    def get(entry):
        at, shape, dtype = entry
        return data[dtype][at:at + int(np.prod(shape, dtype=np.int64))].reshape(shape)
    return index, get


class FakeSelector:
    """The selector's two faces the symbol step uses, over in-memory textures (numpy, or DevArrays once ``to_device``)."""

    def __init__(self, textures, files=None, ctx=None):
        self.image_files = list(FILES if files is None else files)
        self.textures = {k: (ctx.to_device(v) if ctx is not None else v) for k, v in textures.items()}

    def texture(self, ctx, image_file):
        return self.textures[os.path.splitext(os.path.basename(str(image_file)))[0]]
