"""GPU: ScoreMap.from_quad_interpolation / fill_by_quad_interpolation(s) and PageTextLineLabelStep (csrc/quad_interp.hip) through
the public API against the reference's outputs (tests/golden/text_line_label.npz) and the numpy restatement
(tests/text_line_label_restate.py), on host and on device-resident destinations; the launch and synchronisation budget; the
refusals of the C entry points; a seeded random loop.  Float planes are compared under == with NaN positions equal (the sign of
a zero is not pinned); masks exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_line_label_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

G = R.Golden()
QUADS, FILLS, STEPS = G.index['quads'], G.index['fills'], G.index['steps']
PLANE_KEYS = dict(text_line_mask='page_text_line_mask', boundary_mask='page_text_line_boundary_mask',
                  text_line_and_boundary_mask='page_text_line_and_boundary_mask',
                  boundary_score_map='page_text_line_boundary_score_map')


def pairs(rows):
    return [tuple(row) for row in rows]


def points_of(quad):
    from vkit_amd.element import Point
    return [Point.create(y=y, x=x) for y, x in quad]


def selector(component):
    from vkit_amd.element import quad_u, quad_v
    return quad_u if component == R.U else quad_v


def score_map_of(plane, device):
    from vkit_amd import _native as N
    from vkit_amd.element import ScoreMap
    return ScoreMap.from_unchecked_mat(N.default_ctx().to_device(plane)) if device else ScoreMap(mat=plane.copy())


# ---- quads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(QUADS))
def test_from_quad_interpolation_equals_the_reference(name):
    from vkit_amd.element import ScoreMap, quad_u, quad_v
    stored = QUADS[name]
    points, want = points_of(pairs(stored['quad'])), G.get(stored['uv'])
    assert R.same_values(R.quad_uv(pairs(stored['quad']))['uv'], want)
    for component, func in ((0, quad_u), (1, quad_v), (0, lambda np_uv: np_uv[:, :, 0]), (1, lambda np_uv: np_uv[:, :, 1])):
        score_map = ScoreMap.from_quad_interpolation(*points, func_np_uv_to_mat=func)
        assert [score_map.box.up, score_map.box.down, score_map.box.left, score_map.box.right] == stored['box']
        assert score_map.mat.dtype == np.float32 and R.same_values(score_map.mat, want[:, :, component]), (name, component)
    seen = []
    ScoreMap.from_quad_interpolation(*points, func_np_uv_to_mat=lambda np_uv: seen.append(np_uv) or np_uv[:, :, 0], is_prob=False)
    assert seen[0].shape == want.shape and seen[0].dtype == np.float32 and R.same_values(seen[0], want)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('name', list(FILLS))
def test_fill_by_quad_interpolation_equals_the_reference(name, device):
    stored = FILLS[name]
    keep = dict(keep_max_value=stored['mode'] == R.KEEP_MAX, keep_min_value=stored['mode'] == R.KEEP_MIN)
    want = G.get(stored['out'])
    one_by_one = score_map_of(G.get(stored['plane']), device)
    for quad_name, component in stored['entries']:
        func = (lambda uv: uv[:, :, 0] * uv[:, :, 1]) if component == 'product' else selector(component)
        one_by_one.fill_by_quad_interpolation(*points_of(pairs(QUADS[quad_name]['quad'])), func_np_uv_to_mat=func, **keep)
    assert one_by_one.on_device == device
    assert R.same_values(one_by_one.mat, want)
    if name == 'product_max':
        return
    batched = score_map_of(G.get(stored['plane']), device)
    batched.fill_by_quad_interpolations([points_of(pairs(QUADS[q]['quad'])) for q, _ in stored['entries']],
                                        [selector(c) for _, c in stored['entries']], **keep)
    assert batched.on_device == device and R.same_values(batched.mat, want)


def test_zero_where_and_one_selector_for_all():
    from vkit_amd.element import Mask, quad_v
    names = ['trapezoid_up', 'trapezoid_down', 'trapezoid_left', 'trapezoid_right']
    keep = np.zeros((64, 96), np.uint8)
    keep[::2, 10:70] = 1
    want = np.ones((64, 96), np.float32)
    for name in names:
        R.quad_fill(want, pairs(QUADS[name]['quad']), R.V, R.KEEP_MIN)
    want[keep == 0] = 0.0
    for device in (False, True):
        score_map = score_map_of(np.ones((64, 96), np.float32), device)
        score_map.fill_by_quad_interpolations([points_of(pairs(QUADS[n]['quad'])) for n in names], quad_v, keep_min_value=True,
                                              zero_where=Mask(mat=keep))
        assert R.same_values(score_map.mat, want)
    with pytest.raises(NotImplementedError):
        score_map.fill_by_quad_interpolations([points_of(pairs(QUADS['convex']['quad']))], lambda uv: uv[:, :, 0])


# ---- the step -----------------------------------------------------------------------------------------------------------
def step_input(lines, shape):
    from vkit_amd import element as E
    from vkit_amd.engine.font import type as FT
    from vkit_amd.pipeline import text_detection as T
    text_lines = [R.build_text_line(line, E, FT, reference=False) for line in lines]
    return T.PageTextLineLabelStepInput(page_text_line_step_output=T.PageTextLineStepOutput(
        page_text_line_collection=T.PageTextLineCollection(height=shape[0], width=shape[1], text_lines=text_lines,
                                                           short_text_line_flags=[False] * len(lines)),
        page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=shape[0], width=shape[1])))


def make_step(flags):
    from vkit_amd.pipeline import text_detection as T
    return T.page_text_line_label_step_factory.create(dict(enable_text_line_mask=flags[0], enable_boundary_mask=flags[1],
                                                           enable_boundary_score_map=flags[2]))


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
@pytest.mark.parametrize('name', list(STEPS))
def test_step_equals_the_reference(name, resident):
    from vkit_amd import _native as N
    stored = STEPS[name]
    shape = tuple(stored['shape'])
    for run in stored['runs']:
        with N.resident(resident):
            out = make_step(run['flags']).run(step_input(stored['lines'], shape), np.random.default_rng(0))
        restated = R.step_planes(stored['lines'], shape, run['flags'])
        for key, attr in PLANE_KEYS.items():
            plane, ref = getattr(out, attr), run['planes'][key]
            assert (plane is None) == (ref is None), (key, run['flags'])
            if plane is None:
                continue
            assert plane.on_device == resident and plane.shape == shape
            assert R.same_values(plane.mat, G.get(ref)) and R.same_values(plane.mat, restated[key]), (key, run['flags'])
        want = stored['collections']
        assert [pairs(R.xy_of(p)) for p in out.page_text_line_polygon_collection.polygons] == [pairs(p) for p in want['polygons']]
        assert R.xy_of(out.page_char_polygon_collection.height_points_up) == pairs(want['char_up'])
    if not stored['lines']:      # no line: the planes that are asked for come back constant
        assert not out.page_text_line_mask.mat.any() and not G.get(stored['runs'][0]['planes']['boundary_score_map']).any()


def _count(monkeypatch, ctx, call):
    from vkit_amd import _native as N
    syncs = []
    real = N.Context.sync
    ctx.sync()
    with monkeypatch.context() as m:
        m.setattr(N.Context, 'sync', lambda s: syncs.append(1) or real(s))
        ctx.set_timing(1)
        try:
            ctx.reset_timings()
            out = call()
            n_syncs = len(syncs)
            timings = ctx.timings()
        finally:
            ctx.set_timing(0)
    return out, {name: cnt for name, (_ms, cnt) in timings.items()}, n_syncs


def test_launch_and_sync_budget(monkeypatch):
    """1 line and 80: the same launches for all four planes of a page, at most four, no synchronisation"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    step = make_step((True, True, True))
    seen = []
    with N.resident(True):
        for name in ('one_70x131', 'stacked_80_64x96'):
            stored = STEPS[name]
            data = step_input(stored['lines'], tuple(stored['shape']))
            step.run(data, None)         # warm the scratch slots
            out, launches, syncs = _count(monkeypatch, ctx, lambda: step.run(data, None))
            seen.append((launches, syncs))
            run = stored['runs'][0]
            assert R.same_values(out.page_text_line_boundary_score_map.mat, G.get(run['planes']['boundary_score_map']))
    assert seen[0] == seen[1] == ({'k_box_masks': 1, 'k_quad_vote': 1, 'k_quad_fill': 1}, 0), seen
    assert sum(seen[0][0].values()) <= 4
    # the batched fill of the element layer: two launches whatever the number of quads
    from vkit_amd.element import quad_v
    for names in (['convex'], ['convex', 'kite', 'trapezoid_up', 'trapezoid_left', 'slanted']):
        score_map = score_map_of(R.fill_plane(), True)
        quads = [points_of(pairs(QUADS[n]['quad'])) for n in names]
        score_map.fill_by_quad_interpolations(quads, quad_v)
        _, launches, syncs = _count(monkeypatch, ctx, lambda: score_map.fill_by_quad_interpolations(quads, quad_v))
        assert (launches, syncs) == ({'k_quad_vote': 1, 'k_quad_fill': 1}, 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    lib, P = N.lib(), ctypes.c_void_p
    h, w = 40, 60
    dst = ctx.to_device(np.full((h, w), 0.5, np.float32))
    zero = ctx.to_device(np.ones((h, w), np.uint8))
    quad = pairs(QUADS['pixel_tall']['quad'])
    good = N.quad_records([points_of(quad)], N.QUAD_V)
    want = R.quad_fill(np.full((h, w), 0.5, np.float32), quad, R.V, R.PLAIN)

    def clean_call():
        fresh = ctx.to_device(np.full((h, w), 0.5, np.float32))
        N.quad_interp_fill(fresh, good, N.FILL_PLAIN, zero)
        assert R.same_values(fresh.host(), want)

    def fill(recs=good, n=1, mode=0, hh=h, ww=w, d=dst.ptr, z=zero.ptr, handle=ctx.handle):
        return lib.vkx_quad_interp_fill_dev(handle, recs.ctypes.data if recs is not None else None, n, mode, hh, ww, P(d) if d else None,
                                            P(z) if z else None)

    outside = good.copy()
    outside['x'][0, 2] = w
    negative = good.copy()
    negative['y'][0, 0] = -1
    component = good.copy()
    component['component'] = 2
    refused = [
        lambda: fill(handle=None), lambda: fill(d=None), lambda: fill(recs=None),
        lambda: fill(hh=0), lambda: fill(ww=0), lambda: fill(hh=32769), lambda: fill(ww=32769),
        lambda: fill(n=-1), lambda: fill(n=1 << 24),
        lambda: fill(mode=3), lambda: fill(recs=component),
        lambda: fill(recs=outside), lambda: fill(recs=negative),
        lambda: fill(z=dst.ptr), lambda: fill(z=dst.ptr + h * w * 4 - 1),
    ]
    for k, call in enumerate(refused):
        assert call() == N.ERR_INVALID, k
        assert N.last_error()
        clean_call()
    assert (dst.host() == 0.5).all()                       # nothing was launched
    assert fill(recs=None, n=0, z=None) == 0               # no quad, no zeroing plane: nothing to do

    uv = ctx.dev_empty((3, 2, 2), np.float32)
    wide = good.copy()
    wide['x'][0, 1] = wide['x'][0, 0] + 32768

    def uv_call(rec=good, out=uv.ptr, floats=12, handle=ctx.handle):
        return lib.vkx_quad_interp_uv_dev(handle, rec.ctypes.data if rec is not None else None, P(out) if out else None, floats)

    for k, call in enumerate([lambda: uv_call(handle=None), lambda: uv_call(rec=None), lambda: uv_call(out=None),
                              lambda: uv_call(floats=11), lambda: uv_call(rec=wide, floats=2 * 3 * 32769),
                              lambda: uv_call(rec=component)]):
        assert call() == N.ERR_INVALID, k
        clean_call()
    assert uv_call() == 0 and R.same_values(uv.host(), R.quad_uv(quad)['uv'])

    masks = [ctx.dev_empty((h, w), np.uint8) for _ in range(3)]
    boxes = np.array([[2, 3, 4, 5], [10, 10, 6, 8]], np.int32)

    def mask_call(table=boxes, n_text=1, n_dilated=1, hh=h, ww=w, planes=None, handle=ctx.handle):
        planes = planes or [m.ptr for m in masks]
        return lib.vkx_box_label_masks_dev(handle, table.ctypes.data if table is not None else None, n_text, n_dilated, hh, ww,
                                           *(P(p) if p else None for p in planes))

    empty, outside_box = boxes.copy(), boxes.copy()
    empty[1, 2] = 0
    outside_box[0, 1] = w - 4
    for k, call in enumerate([lambda: mask_call(handle=None), lambda: mask_call(table=None), lambda: mask_call(hh=0),
                              lambda: mask_call(ww=32769), lambda: mask_call(n_text=-1), lambda: mask_call(n_dilated=1 << 24),
                              lambda: mask_call(table=empty), lambda: mask_call(table=outside_box),
                              lambda: mask_call(planes=[None, masks[1].ptr, masks[2].ptr]),
                              lambda: mask_call(planes=[masks[0].ptr, masks[0].ptr + 5, masks[2].ptr])]):
        assert call() == N.ERR_INVALID, k
        clean_call()
    assert mask_call() == 0
    text, boundary, both = (m.host() for m in masks)
    want_text = np.zeros((h, w), np.uint8)
    want_text[2:6, 3:8] = 1
    want_both = want_text.copy()
    want_both[10:16, 10:18] = 1
    assert (text == want_text).all() and (both == want_both).all() and (boundary == want_both - want_text).all()


# ---- a seeded random loop -----------------------------------------------------------------------------------------------
def test_random_quads_and_pages_equal_the_restatement():
    from vkit_amd import _native as N
    from vkit_amd.element import ScoreMap
    rng = np.random.default_rng(20240607)
    plane = R.fill_plane((96, 131))
    quads, components = [], []
    while len(quads) < 200:
        side_y, side_x = int(rng.integers(1, 64)), int(rng.integers(1, 64))
        up, left = int(rng.integers(0, 96 - side_y)), int(rng.integers(0, 131 - side_x))
        quad = [(up + float(rng.integers(0, side_y * 4 + 1)) / 4, left + float(rng.integers(0, side_x * 4 + 1)) / 4) for _ in range(4)]
        if rng.integers(0, 3) == 0:          # near-parallelograms: both sides of the |a| < 0.001 threshold and its neighbourhood
            quad[2] = (quad[1][0] + quad[3][0] - quad[0][0] + int(rng.integers(-1, 2)), quad[1][1] + quad[3][1] - quad[0][1])
        (b_up, b_left, bh, bw), rel = R.quad_geometry(quad)
        if tuple(rel[0]) == tuple(rel[3]) or b_up < 0 or b_left < 0 or b_up + bh > 96 or b_left + bw > 131:
            continue
        quads.append(quad)
        components.append(int(rng.integers(0, 2)))
    branches = set()
    for k in range(0, 200, 40):
        got = ScoreMap(mat=R.fill_plane((96, 131)).copy(), is_prob=False)
        got.fill_by_quad_interpolations([points_of(q) for q in quads[k:k + 40]], [selector(c) for c in components[k:k + 40]],
                                        keep_max_value=k % 80 == 0)
        want = plane.copy()
        for quad, component in zip(quads[k:k + 40], components[k:k + 40]):
            R.quad_fill(want, quad, component, R.KEEP_MAX if k % 80 == 0 else R.PLAIN)
            branches.add(R.quad_uv(quad)['branch'])
        assert R.same_values(got.mat, want), k
    assert branches == {'linear', 'pos', 'neg'}
    for k in range(0, 200, 25):              # the raw planes of single quads
        uv = N.quad_interp_uv(N.quad_records([points_of(quads[k])], N.QUAD_V)).host()
        assert R.same_values(uv, R.quad_uv(quads[k])['uv']), k

    step = make_step((True, True, True))
    for page in range(20):
        h, w = int(rng.integers(20, 97)), int(rng.integers(30, 132))
        lines = []
        for _ in range(int(rng.integers(1, 13))):
            is_hori = bool(rng.integers(0, 2))
            thick, long = int(rng.integers(1, 9)), int(rng.integers(4, 40))
            bh, bw = (thick, long) if is_hori else (long, thick)
            bh, bw = min(bh, h - 1), min(bw, w)
            up, left = int(rng.integers(1, h - bh + 1)), int(rng.integers(0, w - bw + 1))
            lines.append(R.make_line((up, up + bh - 1, left, left + bw - 1), is_hori, int(rng.integers(4, 9))))
        with N.resident(page % 2 == 1):
            out = step.run(step_input(lines, (h, w)), None)
        want = R.step_planes(lines, (h, w), (True, True, True))
        for key, attr in PLANE_KEYS.items():
            assert R.same_values(getattr(out, attr).mat, want[key]), (page, key)


# ---- tile borders -------------------------------------------------------------------------------------------------------
BORDER_BOXES = [(8, 32, 8, 32),         # exactly one 32 x 8 tile
                (7, 31, 10, 34),        # one pixel over it on every side
                (44, 69, 1, 1),         # the last pixel
                (0, 0, 45, 70)]         # the whole plane
BORDER_LISTS = [([box], []) for box in BORDER_BOXES] + [([], [box]) for box in BORDER_BOXES] + \
               [([], []), (BORDER_BOXES[:1] + BORDER_BOXES[2:3], BORDER_BOXES[1:2]), (BORDER_BOXES[1:2], BORDER_BOXES[:1] + BORDER_BOXES[2:3])]


@pytest.mark.parametrize('case', range(len(BORDER_LISTS)))
def test_box_masks_at_the_tile_borders(case):
    """vkx_box_label_masks_dev on a 45 x 70 plane (6 x 3 tiles of 32 x 8, ragged last row and column): each box alone as a text
    box and alone as a dilated box, both lists empty, and two mixed lists, against the numpy union of the rectangles."""
    from vkit_amd import _native as N
    h, w = 45, 70
    text_boxes, dilated_boxes = BORDER_LISTS[case]
    want_text, want_dilated = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for want, boxes in ((want_text, text_boxes), (want_dilated, dilated_boxes)):
        for up, left, bh, bw in boxes:
            want[up:up + bh, left:left + bw] = 1
    text, boundary, both = N.box_label_masks((h, w), text_boxes, dilated_boxes)
    assert np.array_equal(text.host(), want_text)
    assert np.array_equal(boundary.host(), want_dilated & (1 - want_text))
    assert np.array_equal(both.host(), want_dilated | want_text)


@pytest.mark.parametrize('mode', [R.PLAIN, R.KEEP_MAX, R.KEEP_MIN], ids=['plain', 'max', 'min'])
@pytest.mark.parametrize('y0,x0', [(7, 31), (7, 32), (8, 31), (8, 32)])
def test_quad_fill_at_the_tile_borders(y0, x0, mode):
    """vkx_quad_interp_fill_dev on a 40 x 70 plane: the quads of quad_cases() translated so that their bounding boxes start one
    pixel before and exactly at the second tile column (x = 31, 32) and the second tile row (y = 7, 8), all in one call, against
    R.quad_fill one by one.  Every quad of quad_cases() whose bounding box fits the plane from (8, 32) takes part (at most 32 x 38:
    the side trapezoids and strips, the one-row quad and the thin one; the others are wider or taller than what is left)."""
    from vkit_amd import _native as N
    h, w = 40, 70
    quads, components = [], []
    for k, (name, quad) in enumerate(R.quad_cases().items()):
        (up, left, bh, bw), _ = R.quad_geometry(quad)
        if bh > h - 8 or bw > w - 32:
            continue
        quads.append([(y - up + y0, x - left + x0) for y, x in quad])
        components.append(k % 2)
    assert len(quads) >= 6
    want = R.fill_plane((h, w)).copy()
    for quad, component in zip(quads, components):
        assert R.quad_geometry(quad)[0][:2] == (y0, x0)
        R.quad_fill(want, quad, component, mode)
    got = N.default_ctx().to_device(R.fill_plane((h, w)).copy())
    N.quad_interp_fill(got, N.quad_records([points_of(q) for q in quads], np.array(components, np.int32)), mode)
    got = got.host()
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)     # (the one-row quad leaves NaNs)
