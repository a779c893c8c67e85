#!/usr/bin/env python3
"""Regenerates tests/golden/text_line.npz and .json by running THE REFERENCE's own render_text_line_meta
(vkit/engine/font/freetype.py:840-960) with the fake glyph rasteriser of tests/text_line_restate.py on every case of its ``CASES``.

    python tests/golden/make_text_line_golden.py

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that).  Oracle patches, and only
these: cv.resize -> oracle.resize, cv.cvtColor -> drop the fourth channel.  The reference's render_char_glyphs_in_text_line is
wrapped to note its arguments (the trimmed glyphs, the char boxes of the placement and the pasted plane's shape) and is otherwise
left alone; build_char_glyph, the kerning limits, both placements with their rng draws, resize, pad, trim and clean-up are the
reference's code running for real.

Stored, data only (arrays and the JSON index in the .npz, a list of the cases in the .json): per case its parameters, the glyphs
as build_char_glyph left them (image, score map, ascent, pads and reference sizes), the placement's boxes and shape, and the
outcome: 'none', 'value_error' (with numpy's message) or the three planes, the char boxes, the returned interpolation, ``text``,
``font_size``; and the generator's state after the call.
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
import text_line_restate as R  # noqa: E402
from vkit.engine.font import freetype as F, type as FT  # noqa: E402

OUT = os.path.join(HERE, 'text_line')


def main():
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    cv_stub.cvtColor = lambda mat, code: np.ascontiguousarray(mat[:, :, :3])
    seen = {}
    real_paste = F.render_char_glyphs_in_text_line

    def noting_paste(style, text_line_height, text_line_width, char_glyphs, char_boxes):
        seen['shape'] = [int(text_line_height), int(text_line_width)]
        seen['glyphs'] = list(char_glyphs)
        seen['boxes'] = R.box_list(char_boxes)
        return real_paste(style=style, text_line_height=text_line_height, text_line_width=text_line_width, char_glyphs=char_glyphs,
                          char_boxes=char_boxes)
    F.render_char_glyphs_in_text_line = noting_paste

    packed = {}

    def put(array):
        if array is None:
            return None
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    rows = []
    for name in R.CASES:
        case = R.case(name)
        rng = default_rng(case['seed'])
        seen.clear()
        outcome, message, line = 'line', None, None
        try:
            line = F.render_text_line_meta(R.run_config_of(case, FT), None, R.make_renderer(case['kind'], case['size'], F.build_char_glyph), rng,
                                           cv_resize_interpolation_enlarge=case['enlarge'], cv_resize_interpolation_shrink=case['shrink'])
            if line is None:
                outcome = 'none'
        except ValueError as error:
            outcome, message = 'value_error', str(error)
        assert outcome == case['expect'], (name, outcome, message)
        row = dict(name=name, case=case, outcome=outcome, message=message, shape=seen['shape'], boxes=seen['boxes'],
                   glyphs=[dict(image=put(g.image.mat), score=put(g.score_map.mat if g.score_map else None), char=g.char, ascent=g.ascent,
                                pads=[g.pad_up, g.pad_down, g.pad_left, g.pad_right], ref=[g.ref_ascent_plus_pad_up, g.ref_char_height,
                                                                                          g.ref_char_width]) for g in seen['glyphs']],
                   rng_state=rng.bit_generator.state)
        if line is not None:
            assert line.image.box == line.mask.box and line.image.box.up == 0 and line.image.box.left == 0
            row.update(image=put(line.image.mat), mask=put(line.mask.mat), score=put(line.score_map.mat if line.score_map else None),
                       char_boxes=R.box_list(line.char_boxes), interp=int(line.cv_resize_interpolation), text=line.text,
                       font_size=int(line.font_size), is_hori=bool(line.is_hori), n_glyphs=len(line.char_glyphs),
                       glyph_color=[int(v) for v in line.glyph_color])
        rows.append(row)

    np.savez_compressed(OUT + '.npz', index=np.array(json.dumps(dict(cases=rows))), **{k: np.concatenate(v) for k, v in packed.items()})
    with open(OUT + '.json', 'w') as f:
        json.dump(dict(cases=[[r['name'], r['outcome'], r['shape'], len(r['glyphs'])] for r in rows]), f, indent=None, separators=(',', ':'))
        f.write('\n')
    print(OUT, os.path.getsize(OUT + '.npz'), '+', os.path.getsize(OUT + '.json'), 'bytes;', len(rows), 'cases;',
          {o: sum(r['outcome'] == o for r in rows) for o in ('line', 'none', 'value_error')})


if __name__ == '__main__':
    main()
