"""numpy restatement of PageTextRegionCroppingStep (reference: pipeline/text_detection/page_text_region_cropping.py) for the
tests, with no GPU: the label selection as plain array compares (closed bounds: a shapely box intersects a point on its
edge), the windows (vkit_amd's CropperState and rotate, which run on the host), the reference's loop, the label shifting and
downsampling as scalar arithmetic, and the crops of tests/crop_restate.py.

It tells a GPU mismatch apart from a fixture mistake: the restatement equals the fixture on the CPU, the kernels equal the
restatement on the GPU.  Labels are rows: ``keys`` int (n, 2) (tag, char_idx), ``smooth`` float64 (n, 2) (y, x), ``quads``
float64 (n, 4, 2) (y, x) up-left, up-right, down-right, down-left."""
import json
import os

import numpy as np

import crop_restate as CR

LABELS = ('page_char_mask', 'page_char_height_score_map', 'page_char_gaussian_score_map', 'page_char_bounding_box_mask')
PLANES = ('page_image',) + LABELS
IS_PROB = {'page_char_height_score_map': False, 'page_char_gaussian_score_map': True}


def select(windows, centroid, deviate):
    """vkx_region_crop_select_dev: windows int (n, 4) (up, down, left, right), tables int (k, 3) (x, y, char_idx) -> (counts
    int32 (n, 2), [kept centroid indices per window], [kept deviate indices per window]), ascending."""
    windows = np.asarray(windows, np.int64).reshape(-1, 4)
    centroid = np.asarray(centroid, np.int64).reshape(-1, 3)
    deviate = np.asarray(deviate, np.int64).reshape(-1, 3)
    counts = np.zeros((len(windows), 2), np.int32)
    rows_c, rows_d = [], []
    for i, (up, down, left, right) in enumerate(windows.tolist()):
        def inside(t):
            return (left <= t[:, 0]) & (t[:, 0] <= right) & (up <= t[:, 1]) & (t[:, 1] <= down)
        kept_c = np.flatnonzero(inside(centroid))
        kept_d = np.flatnonzero(inside(deviate) & np.isin(deviate[:, 2], centroid[kept_c, 2]))
        rows_c.append(kept_c.astype(np.int32))
        rows_d.append(kept_d.astype(np.int32))
        counts[i] = len(kept_c), len(kept_d)
    return counts, rows_c, rows_d


def tables(keys, smooth):
    """the two int tables (x, y, char_idx) of the labels: rint of the smooth point, as the labels' integer points"""
    keys = np.asarray(keys, np.int64).reshape(-1, 2)
    points = np.array([(round(x), round(y)) for y, x in np.asarray(smooth, np.float64).reshape(-1, 2).tolist()],
                      np.int64).reshape(-1, 2)
    table = np.concatenate([points, keys[:, 1:]], axis=1)
    return table[keys[:, 0] == 0], table[keys[:, 0] == 1]


def window(config, shape, shape_before_rotate, angle, rng):
    """the CropperState of one attempt (:123-158)"""
    from vkit_amd.mechanism.cropper import CropperState
    from vkit_amd.mechanism.distortion import rotate
    common = dict(core_size=config['core_size'], pad_size=config['pad_size'], pad_value=config.get('pad_value', 0))
    if angle == 0:
        return CropperState.create_from_random_proposal(shape=tuple(shape), rng=rng, **common)
    before = CropperState.create_from_random_proposal(shape=tuple(shape_before_rotate), rng=rng, **common)
    result = rotate.distort({'angle': angle}, shapable_or_shape=tuple(shape_before_rotate),
                            point=before.original_box.get_center_point())
    assert tuple(result.shape) == tuple(shape)
    return CropperState.create_from_center_point(shape=tuple(shape), center_point=result.point, **common)


def box4(b):
    return [int(b.up), int(b.down), int(b.left), int(b.right)]


def run(planes, keys, smooth, quads, config, shape_before_rotate, angle, num_cropped_pages, rng):
    """PageTextRegionCroppingStep.run -> (attempts: the boxes of every attempt made, samples: dicts); ``rng`` ends where the
    reference's does.  ``config``: the overrides of the step's config (a dict)."""
    shape = planes['page_image'].shape[:2]
    keys = np.asarray(keys, np.int64).reshape(-1, 2)
    smooth = np.asarray(smooth, np.float64).reshape(-1, 2)
    quads = np.asarray(quads, np.float64).reshape(-1, 4, 2)
    centroid, deviate = tables(keys, smooth)
    of_tag = [np.flatnonzero(keys[:, 0] == tag) for tag in (0, 1)]
    core, pad = config['core_size'], config['pad_size']
    factor = config.get('downsample_labeling_factor', 2) if config.get('enable_downsample_labeling', True) else 0
    num_samples = round(config.get('num_samples_factor_relative_to_num_cropped_pages', 1.0) * num_cropped_pages)
    run_count_max = max(3, 2 * num_samples)
    run_count = 0
    attempts, samples = [], []
    while len(samples) < num_samples and run_count < run_count_max:
        state = window(config, shape, shape_before_rotate, angle, rng)
        attempts.append(box4(state.original_box) + box4(state.target_box) + box4(state.original_core_box))
        run_count += 1
        counts, rows_c, rows_d = select([box4(state.original_core_box)], centroid, deviate)
        if counts[0, 0] < config.get('num_centroid_points_min', 10) or counts[0, 1] < config.get('num_deviate_points_min', 10):
            continue
        oy = state.target_box.up - state.original_box.up
        ox = state.target_box.left - state.original_box.left
        kept = np.concatenate([of_tag[0][rows_c[0]], of_tag[1][rows_d[0]]])
        shifted, down_points = [], []
        for k in kept.tolist():
            y, x = float(smooth[k, 0]) + oy, float(smooth[k, 1]) + ox
            (uly, ulx), _, (dry, drx), _ = quads[k].tolist()
            shifted.append((y, x, int(y), int(x), uly + oy, ulx + ox, dry + oy, drx + ox))
            if factor:
                down_points.append((int(y // factor), int(x // factor), 1, factor))
        sample = dict(attempt=run_count - 1, state=state, target_core_box=box4(state.target_core_box),
                      kept_centroid=rows_c[0].astype(np.int64), kept_deviate=rows_d[0].astype(np.int64),
                      keys=keys[kept], shifted=np.array(shifted, np.float64).reshape(-1, 8),
                      page_image=CR.crop(planes['page_image'], state, fill=config.get('pad_value', 0)))
        for name in LABELS:
            sample[name] = CR.crop(planes[name], state, core_only=True)
        if factor:
            crop_size = core + 2 * pad
            assert crop_size % factor == 0 and pad % factor == 0 and core % factor == 0
            begin, end = pad // factor, pad // factor + core // factor - 1
            sample['down_shape'] = [crop_size // factor] * 2
            sample['down_target_core_box'] = [begin, end, begin, end]
            sample['down_points'] = np.array(down_points, np.int64).reshape(-1, 4)
            for name in LABELS:
                plane = sample[name]
                sample['down_' + name] = (CR.shrink_score_map(plane, factor, IS_PROB[name]) if plane.dtype == np.float32
                                          else CR.shrink_mask(plane, factor))
        samples.append(sample)
    return attempts, samples


def load_golden():
    """tests/golden/text_region_cropping.npz as a list of run dicts with their arrays (and their page's planes) in place."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'text_region_cropping.npz'))
    flats = {k: z[k] for k in z.files if k != 'index'}

    def resolve(v):
        if isinstance(v, list) and len(v) == 3 and isinstance(v[1], list) and isinstance(v[2], str) and v[2] in flats:
            at, shape, dtype = v
            return flats[dtype][at:at + int(np.prod(shape))].reshape(shape)
        if isinstance(v, dict):
            return {k: resolve(x) for k, x in v.items()}
        if isinstance(v, list) and v and isinstance(v[0], dict):
            return [resolve(x) for x in v]
        return v

    index = json.loads(str(z['index']))
    pages = [resolve(p) for p in index['pages']]
    runs = []
    for row in index['runs']:
        run_ = resolve(row)
        run_['planes'] = pages[row['page']]
        runs.append(run_)
    return runs


def rng_state(rng):
    state = rng.bit_generator.state['state']
    return [str(state['state']), str(state['inc'])]


def assert_sample_equal(got, want):
    """a restated (or collected) sample against a golden (or restated) one: every field equal, not close"""
    assert got['attempt'] == want['attempt']
    assert list(got['target_core_box']) == list(want['target_core_box'])
    for name in ('kept_centroid', 'kept_deviate'):
        assert np.asarray(got[name]).tolist() == np.asarray(want[name]).tolist(), name
    assert got['shifted'].shape == want['shifted'].shape and got['shifted'].tobytes() == want['shifted'].tobytes()
    want_planes = want['planes'] if 'planes' in want else want
    got_planes = got['planes'] if 'planes' in got else got
    assert ('down_shape' in got) == ('down_shape' in want)
    names = PLANES + (tuple('down_' + n for n in LABELS) if 'down_shape' in want else ())
    for name in names:
        a, b = np.asarray(got_planes[name]), np.asarray(want_planes[name])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    if 'down_shape' in want:
        assert list(got['down_shape']) == list(want['down_shape'])
        assert list(got['down_target_core_box']) == list(want['down_target_core_box'])
        assert np.asarray(got['down_points']).tolist() == np.asarray(want['down_points']).tolist()
