#!/usr/bin/env python3
"""Regenerates tests/golden/text_line_label.npz by running THE REFERENCE's own ScoreMap.from_quad_interpolation and
fill_by_quad_interpolation (vkit/element/score_map.py:139-283, :562-588), TextLine.to_polygon / get_height_points /
get_char_level_height_points / to_char_polygons (vkit/engine/font/type.py:560-755) and PageTextLineLabelStep
(vkit/pipeline/text_detection/page_text_line_label.py) on the cases of tests/text_line_label_restate.py:

    python tests/golden/make_text_line_label_golden.py

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that); the only patch is the one
make_golden.py applies too: cv.fillPoly is the oracle's.

Stored: per quad case the vertices, the bounding box, the (u, v) planes and the branch the reference took (recovered from its
output: the restatement's other root would differ); per fill case the plane before and after; per step case the line tables, the
collections as smooth (x, y) lists, the boxes, dilated boxes and dilated-only boxes in order, the quads in fill order and the
planes of every flag combination.  Data only, never reference source text.  No plane is larger than 70 x 131.

The writer asserts that every one of the three branches (linear, positive root, negative root) is taken by a stored quad case,
and that a NaN appears only where 0 / 0 is the reference's arithmetic: the quads whose vertices share a row or a column.
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import text_line_label_restate as R  # noqa: E402
from make_text_region_flatten_golden import _fill_poly  # noqa: E402
import vkit.element as E  # noqa: E402
from vkit.engine.font import type as FT  # noqa: E402
from vkit.pipeline.text_detection import page_text_line as PTL  # noqa: E402
from vkit.pipeline.text_detection import page_text_line_label as L  # noqa: E402

OUT = os.path.join(HERE, 'text_line_label.npz')
DEGENERATE = ('one_row', 'one_column')


def points_of(quad):
    return [E.Point.create(y=y, x=x) for y, x in quad]


def main():
    cv_stub.fillPoly = _fill_poly
    warnings.simplefilter('ignore', RuntimeWarning)          # 0 / 0 of the degenerate quads
    packed, index = {}, dict(quads={}, fills={}, steps={})

    def put(array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    quads = R.quad_cases()
    branches = set()
    for name, quad in quads.items():
        # (a (h, w, 2) array is no ScoreMap: the planes are taken one selector at a time, as a caller does)
        u = E.ScoreMap.from_quad_interpolation(*points_of(quad), func_np_uv_to_mat=lambda np_uv: np_uv[:, :, 0])
        v = E.ScoreMap.from_quad_interpolation(*points_of(quad), func_np_uv_to_mat=lambda np_uv: np_uv[:, :, 1])
        uv = np.stack((u.mat, v.mat), axis=-1)
        assert uv.shape[0] <= 64 and uv.shape[1] <= 64 and uv.dtype == np.float32
        assert bool(np.isnan(uv).any()) == (name in DEGENERATE), name
        restated = R.quad_uv(quad)
        assert R.same_values(restated['uv'], uv), name
        branches.add(restated['branch'])
        index['quads'][name] = dict(quad=[list(map(float, p)) for p in quad], uv=put(uv), branch=restated['branch'],
                                    box=[u.box.up, u.box.down, u.box.left, u.box.right])
    assert branches == {'linear', 'pos', 'neg'}, branches

    selectors = {R.U: (lambda np_uv: np_uv[:, :, 0]), R.V: (lambda np_uv: np_uv[:, :, 1])}
    for name, (entries, mode) in R.fill_cases().items():
        plane = R.fill_plane()
        score_map = E.ScoreMap(mat=plane.copy())
        for quad_name, component in entries:
            score_map.fill_by_quad_interpolation(*points_of(quads[quad_name]), func_np_uv_to_mat=selectors[component],
                                                 keep_max_value=mode == R.KEEP_MAX, keep_min_value=mode == R.KEEP_MIN)
        assert not np.isnan(score_map.mat).any()
        index['fills'][name] = dict(entries=[[q, c] for q, c in entries], mode=mode, plane=put(plane), out=put(score_map.mat))
    # the arbitrary callable of the tests
    score_map = E.ScoreMap(mat=R.fill_plane().copy())
    score_map.fill_by_quad_interpolation(*points_of(quads['convex']), func_np_uv_to_mat=lambda np_uv: np_uv[:, :, 0] * np_uv[:, :, 1],
                                         keep_max_value=True)
    index['fills']['product_max'] = dict(entries=[['convex', 'product']], mode=R.KEEP_MAX, plane=put(R.fill_plane()),
                                         out=put(score_map.mat))

    for name, case in R.step_cases().items():
        shape = case['shape']
        assert shape[0] <= 70 and shape[1] <= 131
        text_lines = [R.build_text_line(line, E, FT, reference=True) for line in case['lines']]
        collection = PTL.PageTextLineCollection(height=shape[0], width=shape[1], text_lines=text_lines,
                                                short_text_line_flags=[False] * len(text_lines))
        step_input = L.PageTextLineLabelStepInput(page_text_line_step_output=PTL.PageTextLineStepOutput(
            page_text_line_collection=collection,
            page_seal_impression_text_line_collection=PTL.PageSealImpressionTextLineCollection(
                height=shape[0], width=shape[1], seal_impressions=[], seal_impression_resources=[])))
        entry = dict(shape=list(shape), lines=case['lines'], runs=[])
        for flags in case['flags']:
            step = L.PageTextLineLabelStep(L.PageTextLineLabelStepConfig(
                enable_text_line_mask=flags[0], enable_boundary_mask=flags[1], enable_boundary_score_map=flags[2]))
            recorded = []
            real = E.ScoreMap.fill_by_quad_interpolation

            def recording(self, point0, point1, point2, point3, **kwargs):
                recorded.append([[p.smooth_y, p.smooth_x] for p in (point0, point1, point2, point3)])
                return real(self, point0, point1, point2, point3, **kwargs)

            E.ScoreMap.fill_by_quad_interpolation = recording
            try:
                out = step.run(step_input, np.random.default_rng(0))
            finally:
                E.ScoreMap.fill_by_quad_interpolation = real
            planes = dict(text_line_mask=out.page_text_line_mask, boundary_mask=out.page_text_line_boundary_mask,
                          text_line_and_boundary_mask=out.page_text_line_and_boundary_mask,
                          boundary_score_map=out.page_text_line_boundary_score_map)
            for plane in planes.values():
                assert plane is None or not np.isnan(plane.mat).any()
            entry['runs'].append(dict(flags=list(flags), quads=recorded,
                                      planes={key: None if plane is None else put(plane.mat) for key, plane in planes.items()}))
            chars, lines = out.page_char_polygon_collection, out.page_text_line_polygon_collection
            entry['collections'] = dict(
                polygons=[R.xy_of(p) for p in lines.polygons], group_sizes=list(lines.height_points_group_sizes),
                line_up=R.xy_of(lines.height_points_up), line_down=R.xy_of(lines.height_points_down),
                char_polygons=[R.xy_of(p) for p in chars.char_polygons],
                adjusted_char_polygons=[R.xy_of(p) for p in chars.adjusted_char_polygons],
                char_up=R.xy_of(chars.height_points_up), char_down=R.xy_of(chars.height_points_down))
        step = L.PageTextLineLabelStep(L.PageTextLineLabelStepConfig())
        boxes, dilated = step.generate_text_line_boxes_and_dilated_boxes(collection)
        entry['boxes'] = [R.box_tuple(b) for b in boxes]
        entry['dilated_boxes'] = [R.box_tuple(b) for b in dilated]
        entry['dilated_only_boxes'] = [[R.box_tuple(o) for o in step.generate_dilated_only_boxes(b, d)] for b, d in zip(boxes, dilated)]
        index['steps'][name] = entry

    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(index))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print(OUT, size, 'bytes', len(index['quads']), 'quad cases', len(index['fills']), 'fill cases', len(index['steps']), 'step cases')


if __name__ == '__main__':
    main()
