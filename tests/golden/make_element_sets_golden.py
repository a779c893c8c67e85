#!/usr/bin/env python3
"""Regenerates tests/golden/element_sets.npz by running THE REFERENCE's own Mask.from_boxes / from_polygons / from_masks /
from_score_maps (vkit/element/mask.py:153-244) and the fill_by_* families of Image, Mask and ScoreMap
(vkit/element/image.py:371-665, mask.py:283-410, score_map.py:315-520) on the cases of tests/element_sets_restate.py:

    python tests/golden/make_element_sets_golden.py

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that); the only patch is the one
make_golden.py applies too: cv.fillPoly is the oracle's.

Cases (planes of 40 x 50): every constructor in every mode, on a shape and relative to a Box, and on an empty list; every
fill_by_* family of every destination type (Image uint8 with 3 channels and with 1, Mask, ScoreMap) in every mode, with one
value for the whole list (the plural forms) and with a value an element (scalar, tuple, array and element values in turn), image
fills with alpha 1.0, 0.5 and an alpha plane, mask and score-map fills plain, keep_max_value and keep_min_value; an empty list
per destination.  Stored: the inputs (tables and planes), every output, and for the mixed cases the decision of the reference's
uniqueness check.  Data only, never reference source text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import element_sets_restate as R  # noqa: E402
from make_text_region_flatten_golden import _fill_poly  # noqa: E402
import vkit.element as E  # noqa: E402
from vkit.element.uniqueness import check_elements_uniqueness  # noqa: E402

OUT = os.path.join(HERE, 'element_sets.npz')


def main():
    cv_stub.fillPoly = _fill_poly
    packed, index = {}, dict(from_cases=[], fill_cases=[])

    def put(array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    def put_elements(kind, elements):
        if kind == R.BOXES:
            return [list(e) for e in elements]
        if kind == R.POLYGONS:
            return [put(e) for e in elements]
        return [dict(mat=put(mat), box=box and list(box)) for mat, box in elements]

    for case in R.from_cases():
        mask = R.run_from(E, case)
        assert mask.mat.shape[0] <= 64 and mask.mat.shape[1] <= 64
        index['from_cases'].append(dict(name=case['name'], elements=put_elements(case['kind'], case['elements']), out=put(mask.mat),
                                        box=None if mask.box is None else [mask.box.up, mask.box.down, mask.box.left, mask.box.right]))
    for case in R.fill_cases():
        dest = R.run_fill(E, case)
        unique = None
        if not case['unique']:
            values = [R.build_value(E, case, spec) for spec in case['values']]
            unique = bool(check_elements_uniqueness(values))
            if case['dest'].startswith('image') and case['kind'] != R.SCORE_MAPS:
                shape = case['plane'].shape[:2]
                alphas = [R.alpha_of(case, i, R.box_of(case['kind'], raw, shape), False) for i, raw in enumerate(case['elements'])]
                unique = bool(E.Image.check_values_and_alphas_uniqueness(values, alphas))
        index['fill_cases'].append(dict(name=case['name'], plane=put(case['plane']), elements=put_elements(case['kind'], case['elements']),
                                        out=put(dest.mat), unique=unique))
    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(index))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes', len(index['from_cases']), 'constructor cases', len(index['fill_cases']), 'fill cases')


if __name__ == '__main__':
    main()
