#!/usr/bin/env python3
"""Regenerates tests/golden/seal_impression.npz and .json by running THE REFERENCE's own fill_text_line_to_seal_impression and
SealImpressionEllipseEngine (vkit/engine/seal_impression/) on small synthetic inputs.

    python tests/golden/make_seal_impression_golden.py

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that).  Oracle patches, and only
these: cv.resize -> oracle.resize, cv.warpAffine -> oracle.warp_affine, cv.ellipse -> oracle.ellipse_outline on a scratch plane
whose touched pixels are then assigned the call's colour; Image.from_file reads the two in-memory icons (iolite is absent);
cattrs.structure stands in as ``cls(**mapping)``.  The reference's TextLine / CharGlyph objects are built from the blocky
arrays of tests/seal_impression_restate.py (``CASES``); everything else -- the slot walk, the two breaks, the resized width, the
rotation, the out-of-bound skip, the keep-max fill, the internal line, the rescale, every draw of the engine -- is the
reference's code running for real.

Stored, data only (arrays and the JSON index in the .npz, a list of the cases in the .json): per fill case the inputs, the score map, the char polygons and how many chars were placed; per engine run
the config overrides, the seed, alpha, colour, rough placements, slots (angles and points), border style and thickness, the
double line's gap, the icon box, the internal box, the background mask (small seals only) and the generator's state after the
run; per seed also the state after each sampling method called on its own.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import oracle as O  # noqa: E402
import seal_impression_restate as R  # noqa: E402
from vkit.utility import opt as ref_opt  # noqa: E402
from vkit.element import Box, Image, Mask, Point, ScoreMap  # noqa: E402
from vkit.engine.font import type as FT  # noqa: E402
from vkit.engine.image import selector as RS  # noqa: E402
from vkit.engine.seal_impression import ellipse as E, text_line_slot_filler as F  # noqa: E402
from vkit.engine.seal_impression.type import CharSlot, SealImpression, SealImpressionEngineRunConfig, TextLineSlot  # noqa: E402

OUT = os.path.join(HERE, 'seal_impression')

# engine runs: (name, init overrides, with icon folder, (height, width), seeds, keep the background mask)
SMALL = ((40, 40), (64, 96), (33, 51))
ENGINE = []
for _shape in SMALL:
    ENGINE.append(('default', dict(), False, _shape, tuple(range(6)), True))
    ENGINE.append(('thick', dict(border_thickness_ratio_max=0.2), False, _shape, tuple(range(6)), True))
    ENGINE.append(('thick_icon', dict(border_thickness_ratio_max=0.2, prob_add_icon=0.8), True, _shape, tuple(range(6)), True))
ENGINE.append(('large', dict(), False, (256, 256), tuple(range(12)), False))
ENGINE.append(('large_wide_icon', dict(prob_add_internal_text_line=1.0), True, (200, 320), tuple(range(8)), False))
ENGINE.append(('tall', dict(), False, (120, 90), tuple(range(6)), False))


def make_icons():
    rng = default_rng(20240901)
    return {'a.png': (R.blocky(rng, (24, 30), 4, 0, 2, np.uint8) * np.uint8(255)),
            'b.png': (R.blocky(rng, (17, 13), 3, 0, 4, np.uint8) * np.uint8(80))}


def ref_seal(case):
    seal = case['seal']
    slots = [TextLineSlot(text_line_height=s['height'], char_aspect_ratio=s['aspect'],
                          char_slots=[CharSlot(angle=c[0], point_up=Point.create(y=c[1], x=c[2]), point_down=Point.create(y=c[3], x=c[4]))
                                      for c in s['chars']]) for s in seal['slots']]
    box = seal['internal_box']
    return SealImpression(alpha=seal['alpha'], color=(200, 0, 0), background_mask=Mask.from_shape((seal['h'], seal['w'])),
                          text_line_slots=slots,
                          internal_text_line_box=None if box is None else Box(up=box[0], down=box[1], left=box[2], right=box[3]))


def ref_glyph(char):
    return FT.CharGlyph(char='x', image=Image(mat=char['image']), score_map=None if char.get('score') is None else ScoreMap(mat=char['score']),
                        ascent=0, pad_up=0, pad_down=0, pad_left=0, pad_right=0, ref_ascent_plus_pad_up=0,
                        ref_char_height=char['ref_h'], ref_char_width=char['ref_w'])


def ref_line(line, internal=False):
    h, w = line['height'], line['width']
    box = Box(up=0, down=h - 1, left=0, right=w - 1)
    char_boxes = [FT.CharBox(char='x', box=Box(up=c['box'][0], down=c['box'][1], left=c['box'][2], right=c['box'][3])) for c in line['chars']]
    if internal:
        glyphs = [ref_glyph(dict(image=np.zeros((c['box'][1] - c['box'][0] + 1, 3), np.uint8), ref_h=c['ref_h'], ref_w=c['ref_w']))
                  for c in line['chars']]
        mask = Mask(mat=line['mask'], box=box)
        score_map = None if line['score'] is None else ScoreMap(mat=line['score'], box=box)
    else:
        glyphs = [ref_glyph(c) for c in line['chars']]
        mask = Mask(mat=np.ones((h, w), np.uint8), box=box)
        score_map = None
    return FT.TextLine(image=Image(mat=np.zeros((h, w, 3), np.uint8), box=box), mask=mask, score_map=score_map, char_boxes=char_boxes,
                       char_glyphs=glyphs, cv_resize_interpolation=line.get('interp', 2), style=None, font_size=h, text='x' * len(char_boxes),
                       is_hori=True)


def polygons_xy(polygons):
    return [np.array([(p.smooth_x, p.smooth_y) for p in polygon.points], np.float64) for polygon in polygons]


def _ellipse(mat, center, axes, angle, startAngle, endAngle, color, thickness):
    assert (angle, startAngle, endAngle) == (0, 0, 360)
    touched = O.ellipse_outline(np.zeros(mat.shape, np.uint8), center, axes, thickness)
    writeable = mat.flags.writeable       # (the reference draws onto the mask's own array; cv2 does not look at numpy's write flag)
    mat.flags.writeable = True
    mat[touched > 0] = color
    mat.flags.writeable = writeable
    _ellipse.calls.append([int(thickness), [int(a) for a in axes], int(color)])


def main():
    icons = make_icons()
    _ellipse.calls = []
    cv_stub.warpAffine = lambda mat, trans_mat, dsize: O.warp_affine(mat, trans_mat, dsize)
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    cv_stub.ellipse = lambda mat, center, axes, angle, startAngle, endAngle, color, thickness: _ellipse(
        mat, center, axes, angle, startAngle, endAngle, color, thickness)
    ref_opt._cattrs.structure = lambda mapping, cls: cls(**mapping)
    Image.from_file = classmethod(lambda cls, path, disable_exif_orientation=False: cls(mat=icons[os.path.basename(str(path))].copy()))
    choices = []
    real_choice = E.rng_choice
    E.rng_choice = RS.rng_choice = lambda rng, items, probs=None: choices.append(real_choice(rng, items, probs=probs)) or choices[-1]

    packed = {}

    def put(array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    def put_char(c):
        return dict(box=c['box'], score=None if c.get('score') is None else put(c['score']),
                    image=None if c.get('image') is None else put(c['image']), ref_h=c['ref_h'], ref_w=c['ref_w'])

    # ---- the fill
    fills, seen, placed = [], 0, 0
    for name in R.CASES:
        case = R.case(name)
        internal = case['internal']
        stats = {}
        R.fill(case, stats)              # (counts only: which chars the skip rule lets through)
        score_map, polygons = F.fill_text_line_to_seal_impression(
            ref_seal(case), case['indices'], [ref_line(line) for line in case['lines']],
            None if internal is None else ref_line(internal, internal=True))
        n_internal = 0 if internal is None else len(internal['chars'])
        n_placed = len(polygons) - n_internal
        assert n_placed == stats.get('placed', 0), (name, n_placed, stats)
        seen += stats.get('chars', 0)
        placed += n_placed
        if name == 'out_of_bound':
            assert 1 <= n_placed < stats['chars'], (n_placed, stats)
        if name == 'all_zero':
            assert n_placed == 0 and np.isnan(score_map.mat).all()
        fills.append(dict(
            name=name, seal=case['seal'], indices=case['indices'],
            lines=[dict(height=line['height'], width=line['width'], interp=line['interp'], chars=[put_char(c) for c in line['chars']])
                   for line in case['lines']],
            internal=None if internal is None else dict(height=internal['height'], width=internal['width'],
                                                        score=None if internal['score'] is None else put(internal['score']),
                                                        mask=put(internal['mask']), chars=[put_char(c) for c in internal['chars']]),
            score_map=put(score_map.mat), polygons=[put(q) for q in polygons_xy(polygons)], placed=n_placed, chars=stats.get('chars', 0)))
    assert placed >= 0.9 * seen, (placed, seen)

    # ---- the engine
    def plain_point(p):
        return [p.smooth_y, p.smooth_x]

    def plain_slots(text_line_slots):
        return [dict(height=s.text_line_height, aspect=s.char_aspect_ratio,
                     chars=[[c.angle] + plain_point(c.point_up) + plain_point(c.point_down) for c in s.char_slots]) for s in text_line_slots]

    def plain_box(box):
        return None if box is None else [box.up, box.down, box.left, box.right]

    def make_engine(overrides, with_icon):
        config = E.SealImpressionEllipseEngineInitConfig(icon_image_folders=['unused'] if with_icon else None, **overrides)
        engine = E.SealImpressionEllipseEngine(config)
        if with_icon:
            engine.icon_image_selector.engine.image_files = ['icons/a.png', 'icons/b.png']
        return engine

    def double_line_seeds(overrides, with_icon, shape, count=2):
        """the first ``count`` seeds from 100 on whose run erases the middle of its border: at the small sizes that is rare"""
        found = []
        for seed in range(100, 1000):
            del _ellipse.calls[:]
            make_engine(overrides, with_icon).run(SealImpressionEngineRunConfig(height=shape[0], width=shape[1]), default_rng(seed))
            if len(_ellipse.calls) > 1:
                found.append(seed)
                if len(found) == count:
                    break
        return tuple(found)

    runs = []
    for name, overrides, with_icon, shape, seeds, keep_mask in ENGINE:
        if keep_mask and name != 'default':
            seeds = seeds + double_line_seeds(overrides, with_icon, shape)
        for seed in seeds:
            height, width = shape
            engine = make_engine(overrides, with_icon)
            # the sampling methods one by one, on a generator of their own
            rng = default_rng(seed)
            steps = {}
            alpha, color = engine.sample_alpha_and_color(rng)
            steps['alpha_and_color'] = rng.bit_generator.state
            placements = engine.sample_curved_text_line_rough_placements(height, width, rng)
            steps['rough_placements'] = rng.bit_generator.state
            slots = engine.generate_text_line_slots_based_on_rough_placements(height, width, placements, rng)
            steps['text_line_slots'] = rng.bit_generator.state
            inner = (min(p.ellipse_inner_height for p in placements), min(p.ellipse_inner_width for p in placements))
            icon_box = engine.sample_icon_box(height, width, inner, rng)
            steps['icon_box'] = rng.bit_generator.state
            internal_box = engine.sample_internal_text_line_box(height, width, inner, icon_box.down, rng)
            steps['internal_box'] = rng.bit_generator.state
            by_step = dict(icon_box=plain_box(icon_box), internal_box=plain_box(internal_box), states=steps)

            # the whole run
            rng = default_rng(seed)
            del choices[:], _ellipse.calls[:]
            seal = engine.run(SealImpressionEngineRunConfig(height=height, width=width), rng)
            assert (seal.alpha, tuple(seal.color)) == (alpha, tuple(color))
            assert plain_slots(seal.text_line_slots) == plain_slots(slots)
            style = [c for c in choices if isinstance(c, E.SealImpressionEllipseBorderStyle)][0]
            border = _ellipse.calls[0]
            empty = _ellipse.calls[1][0] if len(_ellipse.calls) > 1 else None
            icon_file = [c for c in choices if isinstance(c, str)]
            runs.append(dict(
                case=name, overrides=overrides, with_icon=with_icon, shape=list(shape), seed=seed, alpha=seal.alpha,
                color=[int(v) for v in seal.color], placements=[[p.ellipse_outer_height, p.ellipse_outer_width, p.ellipse_inner_height,
                                                                 p.ellipse_inner_width, p.text_line_height, p.angle_begin, p.angle_end,
                                                                 bool(p.clockwise)] for p in placements],
                slots=plain_slots(seal.text_line_slots), inner=list(inner), border_style=style.value, border_thickness=border[0],
                axes=border[1], border_thickness_empty=empty, icon_file=icon_file[0] if icon_file else None,
                internal_box=plain_box(seal.internal_text_line_box), by_step=by_step,
                background_mask=put(seal.background_mask.mat) if keep_mask else None, rng_state=rng.bit_generator.state))
    small = [r for r in runs if r['background_mask'] is not None]
    assert any(r['border_thickness_empty'] is not None for r in small), 'no double line among the small seals'
    assert any(r['icon_file'] for r in small) and any(r['with_icon'] and not r['icon_file'] for r in small)
    assert all(min(r['axes']) >= 1 for r in small)

    # the arrays and the whole index (one JSON string) in the .npz; the .json lists what the file holds
    np.savez_compressed(OUT + '.npz', icon_a=icons['a.png'], icon_b=icons['b.png'], index=np.array(json.dumps(dict(fills=fills, runs=runs))),
                        **{k: np.concatenate(v) for k, v in packed.items()})
    with open(OUT + '.json', 'w') as f:
        json.dump(dict(fills=[dict(name=r['name'], shape=[r['seal']['h'], r['seal']['w']], chars=r['chars'], placed=r['placed']) for r in fills],
                       runs=[[r['case'], r['shape'][0], r['shape'][1], r['seed']] for r in runs]), f, indent=None, separators=(',', ':'))
        f.write('\n')
    print(OUT, os.path.getsize(OUT + '.npz'), '+', os.path.getsize(OUT + '.json'), 'bytes;', len(fills), 'fills,', len(runs), 'engine runs;',
          placed, 'of', seen, 'chars placed;', sum(r['border_thickness_empty'] is not None for r in runs), 'double lines')


if __name__ == '__main__':
    main()
