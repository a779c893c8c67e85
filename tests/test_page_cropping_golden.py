"""CPU: the crop geometry of vkit_amd.mechanism.cropper and a numpy restatement of PageCroppingStep.run against the
reference's own run (tests/golden/page_cropping.npz)."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_restate as R  # noqa: E402
import cropping_fixture as F  # noqa: E402

CASES = F.cases()
IDS = [f"{c['name']}-{c['seed']}" for c in CASES]


def _config(case):
    from vkit_amd.pipeline.text_detection import PageCroppingStepConfig
    return PageCroppingStepConfig(**case['overrides'])


def test_fixture_covers_the_issue():
    names = {c['name'] for c in CASES}
    assert {'short_axis', 'both_axes', 'crop_sized', 'larger', 'num_samples_set', 'num_samples_clamped', 'text_rejects',
            'active_rejects', 'no_drops', 'no_downsample', 'factor4', 'pad_value', 'is_prob'} <= names
    # runs that end at run_count_max short of num_samples, and page-smaller-than-crop runs that yield nothing at the defaults
    assert any(c['name'] == 'text_rejects' and not c['samples'] and len(c['attempts']) >= 3 for c in CASES)
    assert any(c['name'] == 'short_axis_default' and not c['samples'] for c in CASES)
    assert any(c['name'] == 'short_axis' and c['samples'] for c in CASES)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_cropper_geometry_and_draws(case):
    """Every attempted window, and the generator after the draws, as the reference's."""
    from vkit_amd.element import Box
    from vkit_amd.mechanism.cropper import Cropper, CropperState
    config = _config(case)
    shape = case['planes']['page_image'].shape[:2]
    rng = default_rng(case['seed'])
    for i, want in enumerate(case['attempts']):
        if i == 0:
            cropper = Cropper.create_from_center_point(shape=shape, core_size=config.core_size, pad_size=config.pad_size,
                                                       center_point=Box.from_shape(shape).get_center_point(),
                                                       pad_value=config.pad_value)
        else:
            cropper = Cropper.create_from_random_proposal(shape=shape, core_size=config.core_size, pad_size=config.pad_size,
                                                          rng=rng, pad_value=config.pad_value)
        got = F.box4(cropper.original_box) + F.box4(cropper.target_box) + F.box4(cropper.original_core_box)
        assert got == list(want), i
        assert isinstance(cropper.cropper_state, CropperState)
        assert cropper.crop_size == config.core_size + 2 * config.pad_size
        assert cropper.cropped_shape == (cropper.crop_size,) * 2
        assert cropper.need_post_filling == (cropper.original_box.shape != cropper.cropped_shape)
    assert rng.bit_generator.state == case['rng_state']


def test_sample_cropping_positions_empty_ranges_draw_like_numpy():
    """A page exactly core-sized draws integers(0, 1): whatever numpy consumes for it, the port consumes the same."""
    from vkit_amd.mechanism.cropper import CropperState
    a, b = default_rng(5), default_rng(5)
    CropperState.sample_cropping_positions(height=16, width=40, core_size=16, pad_size=4, crop_size=24, rng=a)
    b.integers(0, 1)
    b.integers(0, 40 - 16 + 1)
    assert a.bit_generator.state == b.bit_generator.state


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_restatement_equals_the_reference(case):
    config = _config(case)
    rng = default_rng(case['seed'])
    got = R.run(case['planes'], config, rng, F.is_prob_of(case))
    assert rng.bit_generator.state == case['rng_state']
    assert len(got) == len(case['samples'])
    for g, want in zip(got, case['samples']):
        assert F.box4(g['state'].target_core_box) == list(want['target_core_box'])
        for name in ('page_image',) + R.LABELS:
            assert g[name].dtype == want[name].dtype and np.array_equal(g[name], want[name]), name
        assert ('down_page_char_mask' in g) == ('down_page_char_mask' in want)
        for name in R.LABELS:
            if 'down_' + name in want:
                a, b = g['down_' + name], want['down_' + name]
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
