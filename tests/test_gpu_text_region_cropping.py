"""PageTextRegionCroppingStep on the GPU (vkit_amd/pipeline/text_detection/page_text_region_cropping.py, csrc/region_crop.hip):
the step against the reference's own runs (tests/golden/text_region_cropping.npz) on host and device pages, the selection
kernel against the restatement (tests/text_region_cropping_restate.py) on random tables, ABI refusals, the launch and
synchronisation budget and the single-attempt form.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_region_cropping_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

RUNS = R.load_golden()
IDS = [f"{r['name']}-{r['seed']}" for r in RUNS]


def _labels(keys, smooth, quads):
    from vkit_amd.element import Point
    from vkit_amd.pipeline.text_detection import PageCharRegressionLabel, PageCharRegressionLabelTag
    tags = (PageCharRegressionLabelTag.CENTROID, PageCharRegressionLabelTag.DEVIATE)
    out = []
    for (tag, g), (y, x), q in zip(np.asarray(keys).tolist(), np.asarray(smooth).tolist(), np.asarray(quads).tolist()):
        corners = [Point.create(y=py, x=px) for py, px in q]
        out.append(PageCharRegressionLabel(char_idx=g, tag=tags[tag], label_point_smooth_y=y, label_point_smooth_x=x,
                                           downsampled_label_point_y=round(y), downsampled_label_point_x=round(x),
                                           up_left=corners[0], up_right=corners[1], down_right=corners[2],
                                           down_left=corners[3]))
    return out


def _input(planes, labels, shape_before_rotate, angle, num_cropped_pages, resident):
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection import (PageCroppingStepOutput, PageTextRegionCroppingStepInput,
                                                  PageTextRegionLabelStepOutput, PageTextRegionStepOutput)
    arrs = {name: np.ascontiguousarray(planes[name]) for name in R.PLANES}
    if resident:
        ctx = N.default_ctx()
        arrs = {name: ctx.to_device(a) for name, a in arrs.items()}
    shape = planes['page_image'].shape[:2]
    return PageTextRegionCroppingStepInput(
        page_cropping_step_output=PageCroppingStepOutput(cropped_pages=[None] * num_cropped_pages),
        page_text_region_step_output=PageTextRegionStepOutput(
            page_image=Image(mat=arrs['page_image']), page_active_mask=Mask(mat=np.ones(shape, np.uint8)),
            page_char_polygons=[], page_text_region_polygons=[], page_char_polygon_text_region_polygon_indices=[],
            shape_before_rotate=tuple(shape_before_rotate), rotate_angle=angle, debug=None),
        page_text_region_label_step_output=PageTextRegionLabelStepOutput(
            page_char_mask=Mask(mat=arrs['page_char_mask']),
            page_char_height_score_map=ScoreMap(mat=arrs['page_char_height_score_map'], is_prob=False),
            page_char_gaussian_score_map=ScoreMap(mat=arrs['page_char_gaussian_score_map']),
            page_char_regression_labels=labels,
            page_char_bounding_box_mask=Mask(mat=arrs['page_char_bounding_box_mask'])))


def _collect(sample, resident):
    """a CroppedPageTextRegion in the restatement's sample form (without the attempt number)"""
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection.page_text_region_cropping import CroppedPageTextRegion
    assert isinstance(sample, CroppedPageTextRegion)
    out = sample.page_char_regression_labels
    got = dict(target_core_box=R.box4(sample.target_core_box), planes={'page_image': sample.page_image.mat})
    assert isinstance(sample.page_image.arr, N.DevArray) == resident
    got['shifted'] = np.array([(lb.label_point_smooth_y, lb.label_point_smooth_x, lb.downsampled_label_point_y,
                                lb.downsampled_label_point_x, lb.up_left.smooth_y, lb.up_left.smooth_x, lb.down_right.smooth_y,
                                lb.down_right.smooth_x) for lb in out], np.float64).reshape(-1, 8)
    got['keys'] = [(int(lb.tag.value == 'deviate'), lb.char_idx) for lb in out]
    assert all(not lb.is_downsampled and lb.valid for lb in out)
    for name in R.LABELS:
        element = getattr(sample, name)
        assert element.box == sample.target_core_box and isinstance(element.arr, N.DevArray) == resident, name
        got['planes'][name] = element.mat
    d = sample.downsampled_label
    if d is not None:
        got['down_shape'] = list(d.shape)
        got['down_target_core_box'] = R.box4(d.target_core_box)
        got['down_points'] = np.array([(lb.downsampled_label_point_y, lb.downsampled_label_point_x, int(lb.is_downsampled),
                                        lb.downsample_labeling_factor) for lb in d.page_char_regression_labels],
                                      np.int64).reshape(-1, 4)
        # a downsampled label keeps the shifted label's smooth point and corners
        assert [(lb.label_point_smooth_y, lb.label_point_smooth_x) for lb in d.page_char_regression_labels] == \
            [(lb.label_point_smooth_y, lb.label_point_smooth_x) for lb in out]
        for name in R.LABELS:
            element = getattr(d, name)
            assert element.box is None
            got['planes']['down_' + name] = element.mat
    return got


def _assert_step_sample(got, want, keys):
    """``got`` from _collect against a golden or restated sample: the kept labels by their keys and order, then every field"""
    of_tag = [np.flatnonzero(keys[:, 0] == tag) for tag in (0, 1)]
    kept = np.concatenate([of_tag[0][np.asarray(want['kept_centroid'], np.int64)],
                           of_tag[1][np.asarray(want['kept_deviate'], np.int64)]])
    assert got['keys'] == [tuple(k) for k in keys[kept].tolist()]
    got = dict(got, attempt=want['attempt'], kept_centroid=want['kept_centroid'], kept_deviate=want['kept_deviate'])
    R.assert_sample_equal(got, want)


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('run', RUNS, ids=IDS)
def test_step_equals_the_reference(run, resident):
    from vkit_amd.pipeline.text_detection import page_text_region_cropping_step_factory as F
    labels = _labels(run['label_key'], run['label_smooth'], run['label_quad'])
    step = F.create(dict(run['config']))
    rng = default_rng(run['seed'])
    out = step.run(_input(run['planes'], labels, run['shape_before_rotate'], run['angle'], run['num_cropped_pages'], resident), rng)
    assert R.rng_state(rng) == run['rng_state']
    assert len(out.cropped_page_text_regions) == len(run['samples'])
    for sample, want in zip(out.cropped_page_text_regions, run['samples']):
        _assert_step_sample(_collect(sample, resident), want, run['label_key'])


def _random_tables(rng, n_windows, n_centroid, n_deviate, span=400, chars=None, gaps=1, duplicates=False):
    chars = chars or max(1, n_centroid)
    a, b = np.sort(rng.integers(-20, span + 20, (2, n_windows, 2)), axis=2)
    windows = np.stack([a[:, 0], a[:, 1], b[:, 0], b[:, 1]], axis=1)
    windows[0] = (-20, span + 20, -20, span + 20)       # the first window holds every label
    tables = []
    for n in (n_centroid, n_deviate):
        t = np.concatenate([rng.integers(0, span, (n, 2)), rng.integers(0, chars, (n, 1)) * gaps], axis=1)
        if duplicates and n:
            t[rng.integers(0, n, n // 2)] = t[rng.integers(0, n, n // 2)]
        tables.append(t)
    return windows.astype(np.int32), tables[0].astype(np.int32), tables[1].astype(np.int32)


SELECT_CASES = {
    'small': dict(n_windows=7, n_centroid=300, n_deviate=500),
    'no deviate labels': dict(n_windows=5, n_centroid=200, n_deviate=0),
    'no centroid labels': dict(n_windows=5, n_centroid=0, n_deviate=200),
    'no labels': dict(n_windows=3, n_centroid=0, n_deviate=0),
    'one window': dict(n_windows=1, n_centroid=1000, n_deviate=1500),
    'one label': dict(n_windows=4, n_centroid=1, n_deviate=1, span=3),
    'strides of 256': dict(n_windows=3, n_centroid=256, n_deviate=512, span=30),
    '4096 windows': dict(n_windows=4096, n_centroid=700, n_deviate=900),
    '100k labels': dict(n_windows=6, n_centroid=100_000, n_deviate=100_000, span=2000),
    'char_idx with gaps': dict(n_windows=9, n_centroid=800, n_deviate=1200, gaps=37),
    'char_idx past the LDS bitmap': dict(n_windows=300, n_centroid=900, n_deviate=1100, gaps=6007, span=60),
    'char_idx 2^24 - 1': dict(n_windows=3, n_centroid=50, n_deviate=80, chars=2, gaps=(1 << 24) - 1, span=20),
    'duplicate points': dict(n_windows=8, n_centroid=600, n_deviate=600, span=40, duplicates=True),
    'few chars': dict(n_windows=8, n_centroid=500, n_deviate=500, chars=5),
}


@pytest.mark.parametrize('name', list(SELECT_CASES))
def test_select_equals_the_restatement(name):
    from vkit_amd import _native as N
    case = SELECT_CASES[name]
    windows, centroid, deviate = _random_tables(default_rng(1000 + list(SELECT_CASES).index(name)), **case)
    want_counts, want_c, want_d = R.select(windows, centroid, deviate)
    counts, rows_c, rows_d = N.region_crop_select(windows, centroid, deviate)
    assert counts.dtype == np.int32 and counts.tolist() == want_counts.tolist()
    # the first window holds every label: no case compares nothing (without centroid labels nothing is kept, by the rule)
    assert want_counts[0].tolist() == [case['n_centroid'], len(want_d[0])]
    assert len(want_d[0]) > 0 or case['n_centroid'] == 0 or case['n_deviate'] == 0
    for got, want in ((rows_c, want_c), (rows_d, want_d)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and g.tolist() == w.tolist()
    # a second call on the same context (the scratch bitmaps of the first are reused) answers the same
    counts2, _, rows_d2 = N.region_crop_select(windows, centroid, deviate)
    assert counts2.tolist() == want_counts.tolist() and all(g.tolist() == w.tolist() for g, w in zip(rows_d2, want_d))


def test_abi_refusals_leave_canaries():
    from vkit_amd import _native as N
    L = N.lib()
    ctx = N.default_ctx()
    windows = np.array([[2, 9, 3, 12], [0, 4, 0, 4]], np.int32)
    centroid = np.array([(5, 5, 0), (3, 2, 1), (20, 20, 2)], np.int32)
    deviate = np.array([(6, 6, 0), (4, 4, 2), (4, 3, 1), (3, 3, 1)], np.int32)
    counts = ctx.to_device(np.full((2, 2), 0x5A5A5A5A, np.int32))
    rows_c = ctx.to_device(np.full((2, 3), 0x5B5B5B5B, np.int32))
    rows_d = ctx.to_device(np.full((2, 4), 0x5C5C5C5C, np.int32))

    def call(w=windows, nw=None, c=centroid, nc=None, d=deviate, nd=None, o=counts, rc=rows_c, rd=rows_d, h=ctx.handle):
        w, c, d = (None if v is None else np.ascontiguousarray(v, np.int32) for v in (w, c, d))
        return L.vkx_region_crop_select_dev(h, w.ctypes.data if w is not None else None, len(w) if nw is None else nw,
                                            c.ctypes.data if c is not None else None, len(c) if nc is None else nc,
                                            d.ctypes.data if d is not None else None, len(d) if nd is None else nd,
                                            o.ptr if o is not None else None, rc.ptr if rc is not None else None,
                                            rd.ptr if rd is not None else None)

    def with_char(table, value):
        table = table.copy()
        table[1, 2] = value
        return table

    cases = {
        'NULL context': lambda: call(h=None),
        'NULL windows': lambda: call(w=None, nw=2),
        'NULL centroid table': lambda: call(c=None, nc=3),
        'NULL deviate table': lambda: call(d=None, nd=4),
        'NULL counts': lambda: call(o=None),
        'NULL centroid rows': lambda: call(rc=None),
        'NULL deviate rows': lambda: call(rd=None),
        'no windows': lambda: call(nw=0),
        '4097 windows': lambda: call(nw=4097),
        'negative centroid count': lambda: call(nc=-1),
        '2^24 deviate labels': lambda: call(nd=1 << 24),
        'negative char_idx': lambda: call(c=with_char(centroid, -1)),
        'char_idx 2^24': lambda: call(d=with_char(deviate, 1 << 24)),
        'down < up': lambda: call(w=[[2, 1, 3, 12], [0, 4, 0, 4]]),
        'right < left': lambda: call(w=[[2, 9, 3, 12], [0, 4, 5, 4]]),
        'counts over the centroid rows': lambda: call(o=rows_c),
        'one table for both rows': lambda: call(rd=rows_c),
        'deviate rows inside the counts': lambda: call(rd=N.DevArray(ctx, counts.ptr + 4, (2, 4), np.int32, 0)),
    }
    for name, fn in cases.items():
        assert fn() == N.ERR_INVALID, name
    ctx.sync()
    for p, v in ((counts, 0x5A5A5A5A), (rows_c, 0x5B5B5B5B), (rows_d, 0x5C5C5C5C)):
        p.invalidate_host()
        assert (p.host() == v).all()
    # and a valid call writes them
    assert call() == 0
    ctx.sync()
    for p in (counts, rows_c, rows_d):
        p.invalidate_host()
    assert counts.host().tolist() == [[2, 3], [1, 2]]
    assert rows_c.host()[0, :2].tolist() == [0, 1] and rows_c.host()[1, :1].tolist() == [1]
    assert rows_d.host()[0, :3].tolist() == [0, 2, 3] and rows_d.host()[1, :2].tolist() == [2, 3]


def _resident_run(run_index=0):
    run = next(r for r in RUNS if r['name'] == 'factor_two' and r['seed'] == run_index)
    labels = _labels(run['label_key'], run['label_smooth'], run['label_quad'])
    return run, labels, _input(run['planes'], labels, run['shape_before_rotate'], run['angle'], run['num_cropped_pages'], True)


def test_device_run_launches_and_syncs(monkeypatch):
    """a device-resident page: two launches (the selection, the crops), one Context.sync, and three copies to the host queued
    before it (the counts and the two index tables); nothing is read back after it, the crops stay on the device"""
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import page_text_region_cropping_step_factory as F
    ctx = N.default_ctx()
    run, labels, step_input = _resident_run()
    step = F.create(dict(run['config']))
    step.run(step_input, default_rng(run['seed']))       # warm the scratch slots
    ctx.sync()
    events = []
    real = {name: getattr(N.Context, name) for name in ('sync', 'sync_stream', 'download', 'download_async', 'copy_out')}
    for name in real:
        monkeypatch.setattr(N.Context, name, (lambda n: lambda s, *a, **k: events.append(n) or real[n](s, *a, **k))(name))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        out = step.run(step_input, default_rng(run['seed']))
        seen = list(events)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    assert {name: cnt for name, (_ms, cnt) in timings.items()} == {'k_region_crop_select': 1, 'k_crop_planes': 1}, timings
    assert seen == ['copy_out', 'copy_out', 'copy_out', 'sync']
    assert len(out.cropped_page_text_regions) == len(run['samples']) == 4
    assert all(isinstance(s.page_image.arr, N.DevArray) for s in out.cropped_page_text_regions)


def test_large_tables_read_only_their_prefixes(monkeypatch):
    """index tables past REGION_CROP_WHOLE_ROWS_MAX: the counts come first, then one copy per non-empty row of exactly its
    count, and a second synchronisation"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    windows, centroid, deviate = _random_tables(default_rng(77), n_windows=40, n_centroid=5000, n_deviate=5000)
    assert 4 * len(windows) * (len(centroid) + len(deviate)) > N.REGION_CROP_WHOLE_ROWS_MAX
    want_counts, want_c, want_d = R.select(windows, centroid, deviate)
    copies, syncs = [], []
    real_copy, real_sync = N.Context.copy_out, N.Context.sync
    monkeypatch.setattr(N.Context, 'copy_out', lambda s, dptr, arr, *a: copies.append(arr.size) or real_copy(s, dptr, arr, *a))
    monkeypatch.setattr(N.Context, 'sync', lambda s: syncs.append(1) or real_sync(s))
    counts, rows_c, rows_d = N.region_crop_select(windows, centroid, deviate, ctx=ctx)
    assert counts.tolist() == want_counts.tolist()
    assert all(g.tolist() == w.tolist() for g, w in zip(rows_c + rows_d, want_c + want_d))
    assert copies == [counts.size] + [int(v) for v in want_counts.T.reshape(-1) if v]
    assert syncs == [1, 1]


@pytest.mark.parametrize('name', ['plain', 'rotate37', 'rejects_most'])
def test_single_attempt_agrees_with_run(name):
    """sample_cropped_page_text_regions on a fresh generator: run's first attempt, its sample or its rejection"""
    from vkit_amd.pipeline.text_detection import PageCharRegressionLabelTag
    from vkit_amd.pipeline.text_detection import page_text_region_cropping_step_factory as F
    for run in (r for r in RUNS if r['name'] == name):
        labels = _labels(run['label_key'], run['label_smooth'], run['label_quad'])
        step_input = _input(run['planes'], labels, run['shape_before_rotate'], run['angle'], run['num_cropped_pages'], True)
        src = step_input.page_text_region_label_step_output
        step = F.create(dict(run['config']))
        rng = default_rng(run['seed'])
        got = step.sample_cropped_page_text_regions(
            page_image=step_input.page_text_region_step_output.page_image, shape_before_rotate=tuple(run['shape_before_rotate']),
            rotate_angle=run['angle'], page_char_mask=src.page_char_mask,
            page_char_height_score_map=src.page_char_height_score_map,
            page_char_gaussian_score_map=src.page_char_gaussian_score_map,
            page_char_bounding_box_mask=src.page_char_bounding_box_mask,
            centroid_page_char_regression_labels=[lb for lb in labels if lb.tag == PageCharRegressionLabelTag.CENTROID],
            deviate_page_char_regression_labels=[lb for lb in labels if lb.tag == PageCharRegressionLabelTag.DEVIATE], rng=rng)
        first = [s for s in run['samples'] if s['attempt'] == 0]
        if not first:
            assert got is None
        else:
            _assert_step_sample(_collect(got, True), first[0], run['label_key'])
        # one attempt's draws were made
        probe = default_rng(run['seed'])
        R.window(run['config'], run['planes']['page_image'].shape[:2], run['shape_before_rotate'], run['angle'], probe)
        assert R.rng_state(rng) == R.rng_state(probe)
