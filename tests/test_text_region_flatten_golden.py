"""CPU: the numpy-plus-oracle restatement of the pixel half of PageTextRegionStep (tests/text_region_flatten_restate.py) against
the reference's own runs (tests/golden/text_region_flatten.npz), bit for bit: every region's planes, boxes and shapes after the
flattening, the resize and the post-rotation, the stacked page and its active mask, and the background."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_region_flatten_restate as R  # noqa: E402

RUNS, BACKGROUND = R.load_golden()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_the_golden_covers_the_cases():
    assert len(RUNS) == 18
    assert {(tuple(r['shape']), r['n']) for r in RUNS} == {(s, n) for s in ((96, 128), (61, 203)) for n in (1, 3, 70)}
    angles = {reg['angle'] for r in RUNS for reg in r['regions']}
    assert angles == {1, 45, 89, 90, 91, 135, 180, 269, 270, 359}
    assert {a for r in RUNS for a in r['post']} == {0, 90, 180, 270}
    assert any(t[0] == 1 for r in RUNS for t in r['targets'])
    shapes = {tuple(reg['mask'].shape) for r in RUNS for reg in r['regions']}
    assert any(h == 1 for h, _ in shapes) and any(w == 1 for _, w in shapes)
    assert any(int(reg['mask'].sum()) == 1 for r in RUNS for reg in r['regions'])


@pytest.mark.parametrize('k', range(len(RUNS)))
def test_restatement_equals_the_reference(k):
    run = RUNS[k]
    page = run['page']
    built = []
    for reg, want in zip(run['regions'], run['built']):
        got = R.flatten(page, reg['mask'], tuple(reg['box']), reg['angle'])
        same(got['image'], want['image'])
        same(got['mask'], want['mask'])
        assert list(got['shape_before_trim']) == want['shape_before_trim']
        assert list(got['rotated_trimmed_box']) == want['rotated_trimmed_box']
        assert list(got['image'].shape[:2]) == want['shape_before_resize']
        built.append(got)
    box = run['regions'][0]['box']
    same(page[box[0]:box[1] + 1, box[2]:box[3] + 1] * (run['regions'][0]['mask'] > 0)[:, :, None], run['text_region_image0'])
    rotated = []
    for i, idx in enumerate(run['keep']):
        image, mask = R.resize_pair(built[idx]['image'], built[idx]['mask'], *run['targets'][i])
        same(image, run['resized'][i]['image'])
        same(mask, run['resized'][i]['mask'])
        if run['post'][i]:
            image, mask = R.post_rotate_pair(image, mask, run['post'][i])
            same(image, run['rotated'][i]['image'])
            same(mask, run['rotated'][i]['mask'])
        rotated.append((image, mask))
    if rotated:
        stack = run['stack']
        image, active = R.stack(stack['image'].shape[:2], rotated, [(b[0], b[2]) for b in stack['boxes']])
        same(image, stack['image'])
        same(active, stack['mask'])


def test_background():
    same(R.background(7, 11), BACKGROUND)
    phase = (np.arange(7)[:, None] + np.arange(11)[None, :]) % 3
    same(((phase[:, :, None] == np.arange(3)) * 255).astype(np.uint8), BACKGROUND)
