"""CPU checks of vkit_amd.engine.seal_impression against tests/golden/seal_impression.npz / .json, the records of the
reference's own fill_text_line_to_seal_impression and SealImpressionEllipseEngine (tests/golden/make_seal_impression_golden.py):
the numpy restatement of the fill (tests/seal_impression_restate.py) equals the goldens bit for bit, and the engine's host
sampling equals the reference's records field for field and leaves the generator in the reference's state.  No GPU, no library."""
import json
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seal_impression_restate as R  # noqa: E402

INDEX, GET = R.golden()


@pytest.mark.parametrize('row', INDEX['fills'], ids=lambda row: row['name'])
def test_restatement_equals_the_golden(row):
    case = R.golden_case(row, GET)
    stats = {}
    score_map, polygons = R.fill(case, stats)
    assert R.same_bits(score_map, GET(row['score_map']))
    assert stats.get('placed', 0) == row['placed'] and stats.get('chars', 0) == row['chars']
    want = [GET(ref) for ref in row['polygons']]
    assert len(polygons) == len(want)
    for got, ref in zip(polygons, want):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


def test_golden_cases_are_the_shared_cases():
    """the file holds the cases of seal_impression_restate.CASES, inputs included, and the .json lists what the .npz holds"""
    assert [row['name'] for row in INDEX['fills']] == list(R.CASES)
    with open(R.GOLDEN + '.json') as f:
        listed = json.load(f)
    assert listed['fills'] == [dict(name=r['name'], shape=[r['seal']['h'], r['seal']['w']], chars=r['chars'], placed=r['placed'])
                               for r in INDEX['fills']]
    assert listed['runs'] == [[r['case'], r['shape'][0], r['shape'][1], r['seed']] for r in INDEX['runs']]
    for row in INDEX['fills']:
        stored, made = R.golden_case(row, GET), R.case(row['name'])
        assert stored['seal'] == made['seal'] and stored['indices'] == made['indices']
        for a, b in zip(stored['lines'], made['lines']):
            assert (a['height'], a['width'], a['interp'], len(a['chars'])) == (b['height'], b['width'], b['interp'], len(b['chars']))
            for ca, cb in zip(a['chars'], b['chars']):
                assert ca['box'] == cb['box'] and ca['image'].tobytes() == cb['image'].tobytes()
                assert (ca['score'] is None) == (cb['score'] is None) and (ca['score'] is None or ca['score'].tobytes() == cb['score'].tobytes())


def test_golden_covers_the_skip_rule():
    rows = {row['name']: row for row in INDEX['fills']}
    assert 1 <= rows['out_of_bound']['placed'] < rows['out_of_bound']['chars']
    assert rows['all_zero']['placed'] == 0 and np.isnan(GET(rows['all_zero']['score_map'])).all()
    assert sum(r['placed'] for r in rows.values()) >= 0.9 * sum(r['chars'] for r in rows.values())
    assert {R.rotate_branch(c[0] - 270) for c in rows['branches']['seal']['slots'][0]['chars']} == {0, 1, 2, 3}
    assert {(c[0] - 270) for c in rows['branches']['seal']['slots'][0]['chars']} >= {0, 90, 180, -270}


class FakeSelector:
    """stands in for the selector image engine: its one draw (the file), no image"""

    def __init__(self, files):
        self.files, self.drawn, self.asked = files, [], []

    def run(self, run_config, rng):
        from vkit_amd.utility import rng_choice
        self.asked.append((run_config['height'], run_config['width']))
        self.drawn.append(rng_choice(rng, self.files))
        return None


def make_engine(run):
    from vkit_amd.engine.seal_impression import SealImpressionEllipseEngine, SealImpressionEllipseEngineInitConfig
    engine = SealImpressionEllipseEngine(SealImpressionEllipseEngineInitConfig(**run['overrides']))
    if run['with_icon']:
        engine.icon_image_selector = FakeSelector(['icons/a.png', 'icons/b.png'])
    return engine


def plain_slots(text_line_slots):
    return [dict(height=s.text_line_height, aspect=s.char_aspect_ratio,
                 chars=[[c.angle, c.point_up.smooth_y, c.point_up.smooth_x, c.point_down.smooth_y, c.point_down.smooth_x] for c in s.char_slots])
            for s in text_line_slots]


def plain_box(box):
    return None if box is None else [box.up, box.down, box.left, box.right]


def plain_placements(placements):
    return [[p.ellipse_outer_height, p.ellipse_outer_width, p.ellipse_inner_height, p.ellipse_inner_width, p.text_line_height,
             p.angle_begin, p.angle_end, bool(p.clockwise)] for p in placements]


def test_at_least_fifty_engine_seeds():
    assert len(INDEX['runs']) >= 50
    assert len({(r['case'], tuple(r['shape']), r['seed']) for r in INDEX['runs']}) == len(INDEX['runs'])


@pytest.mark.parametrize('run', INDEX['runs'], ids=lambda r: f"{r['case']}-{r['shape'][0]}x{r['shape'][1]}-{r['seed']}")
def test_engine_host_sampling_equals_the_reference(run):
    height, width = run['shape']
    engine = make_engine(run)
    rng = default_rng(run['seed'])
    alpha, color = engine.sample_alpha_and_color(rng)
    assert (alpha, list(color)) == (run['alpha'], run['color']) and all(type(v) is int for v in color)
    text_line_slots, inner = engine.generate_text_line_slots(height, width, rng)
    assert plain_slots(text_line_slots) == run['slots'] and list(inner) == run['inner']
    background = engine.sample_background(height, width, inner, rng)
    assert background.border_style.value == run['border_style']
    assert (background.border_thickness, list(background.axes), background.border_thickness_empty) == (
        run['border_thickness'], run['axes'], run['border_thickness_empty'])
    assert background.center == (width // 2, height // 2)
    if run['with_icon']:
        drawn = engine.icon_image_selector.drawn
        assert (drawn[0] if drawn else None) == run['icon_file']
        assert (background.icon_box is None) == (run['icon_file'] is None)
        if background.icon_box is not None:
            assert engine.icon_image_selector.asked == [background.icon_box.shape]
    else:
        assert background.icon_box is None and run['icon_file'] is None
    assert plain_box(background.internal_text_line_box) == run['internal_box']
    assert rng.bit_generator.state == run['rng_state']


@pytest.mark.parametrize('run', INDEX['runs'], ids=lambda r: f"{r['case']}-{r['shape'][0]}x{r['shape'][1]}-{r['seed']}")
def test_engine_sampling_methods_one_by_one(run):
    height, width = run['shape']
    engine = make_engine(run)
    steps = run['by_step']['states']
    rng = default_rng(run['seed'])
    engine.sample_alpha_and_color(rng)
    assert rng.bit_generator.state == steps['alpha_and_color']
    placements = engine.sample_curved_text_line_rough_placements(height, width, rng)
    assert plain_placements(placements) == run['placements'] and rng.bit_generator.state == steps['rough_placements']
    slots = engine.generate_text_line_slots_based_on_rough_placements(height, width, placements, rng)
    assert plain_slots(slots) == run['slots'] and rng.bit_generator.state == steps['text_line_slots']
    inner = tuple(run['inner'])
    icon_box = engine.sample_icon_box(height, width, inner, rng)
    assert plain_box(icon_box) == run['by_step']['icon_box'] and rng.bit_generator.state == steps['icon_box']
    internal_box = engine.sample_internal_text_line_box(height, width, inner, icon_box.down, rng)
    assert plain_box(internal_box) == run['by_step']['internal_box'] and rng.bit_generator.state == steps['internal_box']


def test_char_slot_build_and_type_names():
    from vkit_amd.element import Point
    from vkit_amd.engine import seal_impression as S
    slot = S.CharSlot.build(point_up=Point.create(y=10, x=30), point_down=Point.create(y=20, x=30))
    assert slot.angle == 270 and type(slot.angle) is int
    assert S.CharSlot.build(point_up=Point.create(y=5, x=9), point_down=Point.create(y=5, x=2)).angle == 0
    assert S.SealImpressionEllipseEngine.get_type_name() == 'ellipse'
    assert S.seal_impression_ellipse_engine_executor_factory.get_type_name() == 'ellipse'
    assert 'ellipse' in S.seal_impression_engine_executor_aggregator_factory.type_name_to_engine_executor_factory


def test_new_classes_have_the_assembler_fields():
    """the font TextLine and the engine's SealImpression carry the field names the page assembler's reduced classes have"""
    import attrs
    from vkit_amd.engine.font import TextLine
    from vkit_amd.engine.seal_impression import SealImpression
    from vkit_amd.pipeline.text_detection import page_assembler as A
    assert {f.name for f in attrs.fields(A.TextLine)} <= {f.name for f in attrs.fields(TextLine)} and hasattr(TextLine, 'box')
    assert {f.name for f in attrs.fields(A.SealImpression)} <= {f.name for f in attrs.fields(SealImpression)}
