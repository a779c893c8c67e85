"""The external_ellipse char-mask engine on the GPU (vkit_amd/engine/char_mask/, csrc/char_mask.hip): the engine against
the reference's own runs (tests/golden/char_mask.npz) on host and device planes, PageDistortionStep with the engine against
the restatement (tests/char_mask_restate.py) on its own distorted polygons, ABI refusals, the launch and synchronisation
budget and a seeded soak."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import char_mask_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.load_golden()
ENGINE = [c for c in CASES if c['kind'] == 'engine']
LABELS = [c for c in CASES if c['kind'] == 'labels']


def _polygons(quads):
    from vkit_amd.element import Polygon
    return [Polygon.from_smooth_xy(q) for q in np.asarray(quads, np.float64).reshape(-1, 4, 2)]


def _engine(L):
    from vkit_amd.engine.char_mask import char_mask_engine_executor_aggregator_factory as F
    return F.create_engine_executor({'type': 'external_ellipse', 'config': {'internal_side_length': L}})


def _run_engine(case, resident):
    from vkit_amd import _native as N
    from vkit_amd.element import Box
    from vkit_amd.engine.char_mask import CharMaskEngineRunConfig
    h, w = case['shape']
    boxes = None
    if 'bounds' in case:
        boxes = [Box(up=int(b[0]), down=int(b[1]), left=int(b[2]), right=int(b[3])) for b in case['bounds']]
    config = CharMaskEngineRunConfig(height=h, width=w, char_polygons=_polygons(case['quads']), char_bounding_boxes=boxes)
    with N.resident(resident):
        return _engine(case['L']).run(config)


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', ENGINE, ids=[c['name'] for c in ENGINE])
def test_engine_equals_the_reference(case, resident):
    from vkit_amd import _native as N
    if 'raises' in case:
        with pytest.raises({'RuntimeError': RuntimeError, 'AssertionError': AssertionError}[case['raises']]):
            _run_engine(case, resident)
        return
    out = _run_engine(case, resident)
    assert isinstance(out.combined_chars_mask.arr, N.DevArray) == resident
    assert np.array_equal(out.combined_chars_mask.mat, case['combined'])
    got_boxes = np.asarray([(m.box.up, m.box.down, m.box.left, m.box.right) for m in out.char_masks], np.int32).reshape(-1, 4)
    assert np.array_equal(got_boxes, case['boxes'])
    packed = np.concatenate([m.mat.reshape(-1) for m in out.char_masks]) if out.char_masks else np.zeros(0, np.uint8)
    assert np.array_equal(packed, case['char_masks'])
    assert all(m.mat.shape == m.box.shape for m in out.char_masks)


@pytest.mark.parametrize('L,side,box_side', [(20, 10, 16), (32, 11, 17)])
def test_boxes_at_the_tile_borders(L, side, box_side):
    """axis-aligned square chars whose trimmed boxes are exactly one 16 x 16 tile, and 17 x 17: one pixel into a second tile row and
    column; two overlapping chars, against the restatement"""
    quads = np.array([[(x, y), (x + side, y), (x + side, y + side), (x, y + side)] for x, y in ((30, 20), (38, 25))], np.float64)
    want, chars = R.run(quads, L, (64, 96))
    assert all((down - up + 1, right - left + 1) == (box_side, box_side) for (up, down, left, right), _ in chars)
    out = _run_engine({'shape': (64, 96), 'quads': quads, 'L': L}, True)
    assert np.array_equal(out.combined_chars_mask.mat, want)
    assert [(m.box.up, m.box.down, m.box.left, m.box.right) for m in out.char_masks] == [tuple(box) for box, _ in chars]
    assert all(np.array_equal(m.mat, mat) for m, (_, mat) in zip(out.char_masks, chars))


def test_planes_are_fresh_after_a_refused_call():
    """a raising char leaves no plane behind, and the next call paints as if nothing had happened (ownership planes clean)"""
    bad = next(c for c in ENGINE if c.get('raises') == 'RuntimeError')
    good = next(c for c in ENGINE if 'raises' not in c and c['shape'] == [96, 128])
    with pytest.raises(RuntimeError):
        _run_engine(bad, True)
    out = _run_engine(good, True)
    assert np.array_equal(out.combined_chars_mask.mat, good['combined'])


def _step_pages(seed, size, n_lines, engine_config):
    from vkit_amd.pipeline import text_detection as T
    from vkit_amd.pipeline.text_detection.synthetic_page import synthetic_page_input
    step_input = synthetic_page_input(seed=seed, size=size, n_lines=n_lines)
    rng = default_rng(1000 + seed)
    a = T.page_assembler_step_factory.create().run(step_input, rng)
    config = T.PageDistortionStepConfig(char_mask_engine_config=engine_config)
    return T.PageDistortionStep(config).run(T.PageDistortionStepInput(a), rng)


def _quads_of(polygons):
    from vkit_amd.engine.char_mask.external_ellipse import char_quads
    return char_quads(polygons)


@pytest.mark.parametrize('seed,L', [(0, 40), (1, 20), (2, 33)])
def test_step_labels_equal_the_restatement(seed, L):
    ellipse = _step_pages(seed, 1024, 40, {'type': 'external_ellipse', 'config': {'internal_side_length': L}})
    default = _step_pages(seed, 1024, 40, {'type': 'default'})
    shape = ellipse.page_image.shape
    chars = _quads_of(ellipse.page_char_polygon_collection.char_polygons)
    seal = _quads_of(ellipse.page_seal_impression_char_polygon_collection.char_polygons)
    assert len(chars) > 100
    want_char, _ = R.run(chars, L, shape)
    want_seal, _ = R.run(seal, L, shape)
    assert np.array_equal(ellipse.page_char_mask.mat, want_char)
    assert np.array_equal(ellipse.page_seal_impression_char_mask.mat, want_seal)
    heights = np.asarray(ellipse.page_char_heights, np.float32)
    assert np.array_equal(ellipse.page_char_height_score_map.mat, R.height_map(chars, L, shape, heights))
    # the rest of the page is the default engine's, byte for byte
    assert np.array_equal(ellipse.page_image.mat, default.page_image.mat)
    for name in ('page_text_line_mask', 'page_text_line_height_score_map', 'page_active_mask'):
        assert getattr(ellipse, name).mat.tobytes() == getattr(default, name).mat.tobytes(), name
    assert ellipse.page_char_heights == default.page_char_heights
    assert not np.array_equal(ellipse.page_char_mask.mat, default.page_char_mask.mat)


@pytest.mark.parametrize('case', LABELS, ids=[c['name'] for c in LABELS])
def test_step_labels_equal_the_reference_step(case):
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Point, PointList
    from vkit_amd.pipeline.text_detection.page_distortion import PageDistortionStep, PageDistortionStepConfig
    step = PageDistortionStep(PageDistortionStepConfig(
        char_mask_engine_config={'type': 'external_ellipse', 'config': {'internal_side_length': case['L']}}))
    image = Image(mat=np.zeros(tuple(case['shape']) + (3,), np.uint8))
    up = PointList(Point.create(y=float(y), x=float(x)) for x, y in case['up'])
    down = PointList(Point.create(y=float(y), x=float(x)) for x, y in case['down'])
    with N.resident(True):
        char_mask, seal_mask, height_map, heights, _ = step.generate_char_labelings(
            image, _polygons(case['quads']), _polygons(case['seal']), up, down)
    assert np.array_equal(char_mask.mat, case['char_mask'])
    assert np.array_equal(seal_mask.mat, case['seal_mask'])
    assert np.array_equal(height_map.mat, case['height_map'])
    assert np.array_equal(np.asarray(heights), case['heights'])


def test_device_run_launches_and_syncs(monkeypatch):
    """A device-resident page with the ellipse engine: at most 4 char-mask launches and one library call (its one
    synchronisation) for all ellipse sets of the page."""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    engine_config = {'type': 'external_ellipse', 'config': {'internal_side_length': 40}}
    _step_pages(3, 1024, 40, engine_config)      # warm the scratch slots
    ctx.sync()
    calls = []
    real = N.char_mask_ellipse_sets
    monkeypatch.setattr(N, 'char_mask_ellipse_sets', lambda *a, **k: calls.append(1) or real(*a, **k))
    syncs = []
    real_sync = N.Context.sync
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        out = _step_pages(3, 1024, 40, engine_config)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    launches = sum(n for name, (_ms, n) in timings.items() if name.startswith('k_char_mask'))
    assert calls == [1], calls
    assert 1 <= launches <= 4, timings
    assert set(n for n in timings if n.startswith('k_char_mask')) <= {'k_char_mask_setup', 'k_char_mask_raster', 'k_char_mask_resolve'}
    assert isinstance(out.page_char_mask.arr, N.DevArray) and isinstance(out.page_char_height_score_map.arr, N.DevArray)


def _set(N, quads, mask=None, score=None, values=None, n_points=4, bounds=None, boxes=None):
    quads = np.ascontiguousarray(np.asarray(quads, np.float64).reshape(-1, 2))
    n = quads.shape[0] // n_points
    offsets = np.arange(0, n_points * n + 1, n_points, dtype=np.int32)
    boxes = boxes if boxes is not None else np.full((max(n, 1), 5), -9, np.int32)
    keep = [quads, offsets, boxes]
    rec = N.VkxCharSet()
    rec.pts_host, rec.poly_offsets_host, rec.n_chars = quads.ctypes.data, offsets.ctypes.data, n
    if values is not None:
        values = np.ascontiguousarray(values, np.float32)
        keep.append(values)
        rec.values_host = values.ctypes.data
    if bounds is not None:
        bounds = np.ascontiguousarray(bounds, np.int32)
        keep.append(bounds)
        rec.bounds_host = bounds.ctypes.data
    rec.mask = mask.ptr if mask is not None else None
    rec.score = score.ptr if score is not None else None
    rec.boxes_host = boxes.ctypes.data
    return rec, keep


def test_abi_refusals_leave_canaries():
    from vkit_amd import _native as N
    L = N.lib()
    ctx = N.default_ctx()
    h, w = 40, 50
    mask = ctx.to_device(np.full((h, w), 0xAB, np.uint8))
    score = ctx.to_device(np.full((h, w), 7.5, np.float32))
    sq = np.array([(10, 10), (20, 10), (20, 20), (10, 20)], np.float64)

    def call(sets, side=20, hh=h, ww=w):
        arr = (N.VkxCharSet * len(sets))(*[s for s, _ in sets])
        return L.vkx_char_mask_ellipse_sets_fresh_dev(ctx.handle, side, arr, len(sets), hh, ww)

    cases = {
        'side 0': ([_set(N, sq, mask=mask)], 0),
        'side too large': ([_set(N, sq, mask=mask)], 4096),
        'three points': ([_set(N, sq[:3], mask=mask, n_points=3)], 20),
        'five points': ([_set(N, np.concatenate([sq, sq[:1]]), mask=mask, n_points=5)], 20),
        'score without values': ([_set(N, sq, score=score)], 20),
        'same mask twice': ([_set(N, sq, mask=mask), _set(N, sq, mask=mask)], 20),
        'mask inside score': ([_set(N, sq, score=score, values=[1.0]), _set(N, sq, mask=N.DevArray(ctx, score.ptr + 8, (h, w), np.uint8, 0))], 20),
        'non-finite point': ([_set(N, np.where(sq == 20, np.nan, sq), mask=mask)], 20),
        'bounds outside the page': ([_set(N, sq, mask=mask, bounds=[(0, h, 0, w - 1)])], 20),
        'nine sets': ([_set(N, sq, mask=None) for _ in range(9)], 20),
    }
    for name, (sets, side) in cases.items():
        boxes = [k[2] for _, k in sets]
        assert call(sets, side) == N.ERR_INVALID, name
        assert all((b == -9).all() for b in boxes), name
    assert (mask.host() == 0xAB).all() and (score.host() == np.float32(7.5)).all()
    score.invalidate_host()
    mask.invalidate_host()
    # a raising char: the status comes back, no plane is written
    off = _set(N, sq + 500, mask=mask)
    assert call([off]) == N.ERR_CHAR_MASK and off[1][2][0, 4] == 1
    assert (mask.host() == 0xAB).all()


def test_soak_seeded_pages():
    """300 seeded pages of 40 to 120 chars, rotated / perspective, some crossing the edges: every one equals the
    restatement; bounded time."""
    from vkit_amd import _native as N
    rng = default_rng(77)
    t0 = time.time()
    raised = 0
    for page in range(300):
        h, w = int(rng.integers(64, 200)), int(rng.integers(64, 200))
        L = int(rng.choice([20, 33, 40, 64]))
        n = int(rng.integers(40, 121))
        size = rng.uniform(3, 30, n)
        centre = np.stack([rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)], axis=1)
        base = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64)[None] * (size[:, None, None] / 2)
        a = rng.uniform(-0.7, 0.7, n)
        rot = np.stack([np.stack([np.cos(a), -np.sin(a)], 1), np.stack([np.sin(a), np.cos(a)], 1)], 1)
        quads = np.einsum('nij,nkj->nki', rot, base) + rng.uniform(-0.15, 0.15, (n, 4, 2)) * size[:, None, None]
        quads = np.round(quads + centre[:, None, :], 2)
        mask = N.default_ctx().dev_empty((h, w), np.uint8)
        s = N.CharMaskSet(quads, mask=mask, want_char_masks=True)
        placed = N.char_mask_ellipse_sets(L, [s], (h, w))
        try:
            want, chars = R.run(quads, L, (h, w))
        except (RuntimeError, AssertionError) as e:
            assert not placed
            first = int(np.nonzero(s.boxes[:, 4])[0][0])
            assert R.ERRORS[int(s.boxes[first, 4])] is type(e), page
            raised += 1
            continue
        assert placed, page
        assert np.array_equal(mask.host(), want), page
        assert np.array_equal(s.boxes[:, :4], np.asarray([b for b, _ in chars], np.int32).reshape(-1, 4)), page
        assert np.array_equal(s.char_masks[:s.packed_size()], np.concatenate([m.reshape(-1) for _, m in chars])), page
    assert 0 < raised < 300
    assert time.time() - t0 < 300
