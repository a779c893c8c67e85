"""CPU: the restatement of tests/text_line_label_restate.py equals the reference's own outputs (tests/golden/text_line_label.npz,
written by tests/golden/make_text_line_label_golden.py), and the host half of vkit_amd's TextLine methods and
PageTextLineLabelStep -- collections, box lists, quad tables in order -- equals them too.  Float planes are compared under ==
with NaN positions equal; masks, tables and point lists exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_line_label_restate as R  # noqa: E402

from vkit_amd import _native as N  # noqa: E402
from vkit_amd import element as E  # noqa: E402
from vkit_amd.element import score_map as SM  # noqa: E402
from vkit_amd.engine.font import type as FT  # noqa: E402
from vkit_amd.pipeline import text_detection as T  # noqa: E402

G = R.Golden()
QUADS, FILLS, STEPS = G.index['quads'], G.index['fills'], G.index['steps']


def pairs(rows):
    return [tuple(row) for row in rows]


def test_the_golden_holds_the_cases_of_the_restatement():
    assert list(QUADS) == list(R.quad_cases()) and set(FILLS) == set(R.fill_cases()) | {'product_max'}
    assert list(STEPS) == list(R.step_cases())
    assert {q['branch'] for q in QUADS.values()} == {'linear', 'pos', 'neg'}
    for name, case in R.step_cases().items():
        assert STEPS[name]['lines'] == [dict(line, box=list(line['box']), char_boxes=[list(b) for b in line['char_boxes']],
                                             refs=[list(r) for r in line['refs']]) for line in case['lines']]
        assert [tuple(run['flags']) for run in STEPS[name]['runs']] == [tuple(f) for f in case['flags']]
    shapes = {tuple(step['shape']) for step in STEPS.values()}
    assert shapes == {(64, 96), (70, 131)}
    assert len(STEPS['stacked_80_64x96']['lines']) == 80 and STEPS['empty_64x96']['lines'] == []


@pytest.mark.parametrize('name', list(QUADS))
def test_restated_quad_equals_the_reference(name):
    stored = QUADS[name]
    solved = R.quad_uv(pairs(stored['quad']))
    up, left, bh, bw = solved['box']
    assert [up, up + bh - 1, left, left + bw - 1] == stored['box']
    assert solved['branch'] == stored['branch']
    assert R.same_values(solved['uv'], G.get(stored['uv']))
    assert bool(np.isnan(solved['uv']).any()) == (name in ('one_row', 'one_column'))


@pytest.mark.parametrize('name', list(FILLS))
def test_restated_fill_equals_the_reference(name):
    stored = FILLS[name]
    plane = G.get(stored['plane']).copy()
    assert (plane == R.fill_plane()).all() and len(np.unique(plane)) > 2
    for quad_name, component in stored['entries']:
        quad = pairs(QUADS[quad_name]['quad'])
        if component == 'product':
            R.quad_fill(plane, quad, None, stored['mode'], func=lambda uv: uv[:, :, 0] * uv[:, :, 1])
        else:
            R.quad_fill(plane, quad, component, stored['mode'])
    assert R.same_values(plane, G.get(stored['out']))
    assert bool((plane == R.fill_plane()).all()) == (name == 'nan_plain')       # a NaN is never written


@pytest.mark.parametrize('name', list(STEPS))
def test_restated_step_equals_the_reference(name):
    stored = STEPS[name]
    lines, shape = stored['lines'], tuple(stored['shape'])
    collections = R.step_collections(lines, shape)
    for key, want in stored['collections'].items():
        got = collections[key]
        if key.endswith('polygons'):
            assert [pairs(p) for p in got] == [pairs(p) for p in want], key
        elif key == 'group_sizes':
            assert got == want
        else:
            assert pairs(got) == pairs(want), key
    boxes, dilated = R.step_boxes(lines, shape)
    assert boxes == pairs(stored['boxes']) and dilated == pairs(stored['dilated_boxes'])
    only = [[None if o is None else tuple(o) for o in R.dilated_only_boxes(b, d)] for b, d in zip(boxes, dilated)]
    assert only == [[None if o is None else tuple(o) for o in row] for row in stored['dilated_only_boxes']]
    for run in stored['runs']:
        planes = R.step_planes(lines, shape, run['flags'])
        assert set(planes) == {key for key, ref in run['planes'].items() if ref is not None}
        for key, plane in planes.items():
            assert R.same_values(plane, G.get(run['planes'][key])), (key, run['flags'])
        if run['flags'] == [True, True, True]:
            assert [tuple(map(tuple, q)) for q in R.step_quads(boxes, dilated)] == [tuple(pairs(q)) for q in run['quads']]
        else:
            assert run['quads'] == []


# ---- vkit_amd's host half ---------------------------------------------------------------------------------------------
def amd_lines(lines):
    return [R.build_text_line(line, E, FT, reference=False) for line in lines]


def amd_input(lines, shape):
    return T.PageTextLineLabelStepInput(page_text_line_step_output=T.PageTextLineStepOutput(
        page_text_line_collection=T.PageTextLineCollection(height=shape[0], width=shape[1], text_lines=amd_lines(lines),
                                                           short_text_line_flags=[False] * len(lines)),
        page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=shape[0], width=shape[1])))


@pytest.mark.parametrize('name', list(STEPS))
def test_text_line_methods_equal_the_reference(name):
    stored = STEPS[name]
    want = stored['collections']
    text_lines = amd_lines(stored['lines'])
    assert [pairs(R.xy_of(line.to_polygon())) for line in text_lines] == [pairs(p) for p in want['polygons']]
    ups = [R.xy_of(line.get_height_points(num_points=3, is_up=True)) for line in text_lines]
    downs = [R.xy_of(line.get_height_points(num_points=3, is_up=False)) for line in text_lines]
    assert [len(u) for u in ups] == want['group_sizes']
    assert [p for u in ups for p in u] == pairs(want['line_up']) and [p for d in downs for p in d] == pairs(want['line_down'])
    assert [p for line in text_lines for p in R.xy_of(line.get_char_level_height_points(is_up=True))] == pairs(want['char_up'])
    assert [p for line in text_lines for p in R.xy_of(line.get_char_level_height_points(is_up=False))] == pairs(want['char_down'])


@pytest.mark.parametrize('name', list(STEPS))
def test_step_host_half_equals_the_reference(name):
    stored = STEPS[name]
    shape = tuple(stored['shape'])
    step = T.page_text_line_label_step_factory.create(dict(enable_text_line_mask=True, enable_boundary_mask=True,
                                                           enable_boundary_score_map=True))
    collection = amd_input(stored['lines'], shape).page_text_line_step_output.page_text_line_collection
    chars = step.generate_page_char_polygon_collection(collection)
    lines = step.generate_page_text_line_polygon_collection(collection)
    want = stored['collections']
    assert (chars.height, chars.width, lines.height, lines.width) == shape + shape
    assert [pairs(R.xy_of(p)) for p in lines.polygons] == [pairs(p) for p in want['polygons']]
    assert list(lines.height_points_group_sizes) == want['group_sizes']
    assert R.xy_of(lines.height_points_up) == pairs(want['line_up']) and R.xy_of(lines.height_points_down) == pairs(want['line_down'])
    assert [pairs(R.xy_of(p)) for p in chars.char_polygons] == [pairs(p) for p in want['char_polygons']]
    assert [pairs(R.xy_of(p)) for p in chars.adjusted_char_polygons] == [pairs(p) for p in want['adjusted_char_polygons']]
    assert R.xy_of(chars.height_points_up) == pairs(want['char_up']) and R.xy_of(chars.height_points_down) == pairs(want['char_down'])

    boxes, dilated = step.generate_text_line_boxes_and_dilated_boxes(collection)
    assert [R.box_tuple(b) for b in boxes] == pairs(stored['boxes'])
    assert [R.box_tuple(b) for b in dilated] == pairs(stored['dilated_boxes'])
    only = [[R.box_tuple(o) for o in step.generate_dilated_only_boxes(b, d)] for b, d in zip(boxes, dilated)]
    assert only == [[None if o is None else tuple(o) for o in row] for row in stored['dilated_only_boxes']]

    run = next(run for run in stored['runs'] if run['flags'] == [True, True, True])
    quads = step.generate_boundary_quads(boxes, dilated)
    assert [[[p.smooth_y, p.smooth_x] for p in quad] for quad in quads] == run['quads']
    text_table, only_table, quad_table = step.generate_label_tables(collection)
    assert text_table.tolist() == [[b[0], b[2], b[1] - b[0] + 1, b[3] - b[2] + 1] for b in stored['boxes']]
    flat = [o for row in stored['dilated_only_boxes'] for o in row if o is not None]
    assert only_table.tolist() == [[o[0], o[2], o[1] - o[0] + 1, o[3] - o[2] + 1] for o in flat]
    # the records: integer vertices in page coordinates, float32 vertices relative to the bounding box, all storing v
    assert quad_table.dtype == N.QUAD_DTYPE and len(quad_table) == len(run['quads'])
    for record, quad in zip(quad_table, run['quads']):
        (up, left, _, _), rel = R.quad_geometry(pairs(quad))
        assert record['x'].tolist() == (rel[:, 0] + left).tolist() and record['y'].tolist() == (rel[:, 1] + up).tolist()
        assert record['sx'].tolist() == rel[:, 0].tolist() and record['sy'].tolist() == rel[:, 1].tolist()
        assert record['component'] == N.QUAD_V
    # without the flags the tables are not built
    plain = T.PageTextLineLabelStep(T.PageTextLineLabelStepConfig(enable_text_line_mask=True))
    assert plain.generate_label_tables(collection)[1:] == (None, None)


def test_a_line_in_row_0_fails_as_in_the_reference():
    box, is_hori, font_size = R.TOP_LINE['line']
    collection = amd_input([R.make_line(box, is_hori, font_size)], R.TOP_LINE['shape']).page_text_line_step_output.page_text_line_collection
    step = T.PageTextLineLabelStep(T.PageTextLineLabelStepConfig(enable_text_line_mask=True, enable_boundary_mask=True))
    boxes, dilated = step.generate_text_line_boxes_and_dilated_boxes(collection)
    up_box = step.generate_dilated_only_boxes(boxes[0], dilated[0])[0]
    assert up_box is not None and up_box.height == 0
    with pytest.raises(AssertionError):
        step.generate_label_tables(collection)
    with pytest.raises(AssertionError):
        R.step_planes([R.make_line(box, is_hori, font_size)], R.TOP_LINE['shape'], (True, True, False))
    assert T.PageTextLineLabelStep(T.PageTextLineLabelStepConfig(enable_text_line_mask=True)).generate_label_tables(collection)[1] is None


def test_quad_records_refuse_what_the_reference_cannot_index():
    """point0 and point3 on one pixel: the reference's self-relative polygon drops the closing duplicate and has no points[3]"""
    points = [E.Point.create(y=y, x=x) for y, x in ((4, 9), (4, 2), (4, 2), (4.4, 9.2))]
    with pytest.raises(IndexError):
        N.quad_records([points], N.QUAD_V)


def test_selectors_and_np_vec():
    uv = np.arange(24, dtype=np.float32).reshape(3, 4, 2)
    assert (SM.quad_u(uv) == uv[:, :, 0]).all() and (SM.quad_v(uv) == uv[:, :, 1]).all()
    assert E.quad_u is SM.quad_u and E.quad_v is SM.quad_v
    a, b = SM.NpVec.from_point(E.Point.create(y=2.5, x=1.25)), SM.NpVec.from_point(E.Point.create(y=4, x=3))
    assert a.x.dtype == np.float32 and a.x.ndim == 0
    assert float(a * b) == 1.25 * 4 - 2.5 * 3 and float((a + b).x) == 4.25 and float((b - a).y) == 1.5
    grid = SM.NpVec(x=np.arange(3, dtype=np.int32), y=np.zeros(3, np.int32))
    assert (grid - a).x.dtype == np.float64          # int32 array minus float32 0-d array: what makes q float64
    out = T.PageTextLineLabelStepOutput(page_char_polygon_collection=T.PageCharPolygonCollection(height=1, width=1),
                                        page_text_line_polygon_collection=T.PageTextLinePolygonCollection(height=1, width=1))
    assert (out.page_text_line_mask, out.page_text_line_boundary_mask, out.page_text_line_and_boundary_mask,
            out.page_text_line_boundary_score_map) == (None, None, None, None)


def test_keep_flags_exclude_one_another():
    score_map = E.ScoreMap.from_shape((8, 8))
    points = [E.Point.create(y=y, x=x) for y, x in ((1, 1), (1, 6), (6, 6), (6, 1))]
    with pytest.raises(AssertionError):
        score_map.fill_by_quad_interpolation(*points, func_np_uv_to_mat=SM.quad_v, keep_max_value=True, keep_min_value=True)
