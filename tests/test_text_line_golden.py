"""CPU checks of the font engine's text-line half against tests/golden/text_line.npz, the outputs of the reference's own
render_text_line_meta (tests/golden/make_text_line_golden.py): the numpy restatement of the pixel half equals the goldens bit for
bit, and the package's host planning (glyphs, char boxes, shapes, trim index, interpolation, rng draws) equals them with no device."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_line_restate as R  # noqa: E402

INDEX, GET = R.golden()
ROWS = {row['name']: row for row in INDEX['cases']}


def test_golden_holds_every_case_as_it_is_defined():
    assert list(ROWS) == list(R.CASES)
    for name, row in ROWS.items():
        assert row['case'] == json.loads(json.dumps(R.case(name))), name
        assert row['outcome'] == R.CASES[name]['expect'], name
        across, along = (row['case']['height'], row['case']['width']) if row['case']['hori'] else (row['case']['width'], row['case']['height'])
        assert 12 <= across <= 40 and 16 <= along <= 160, name


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_equals_the_golden(name):
    row = ROWS[name]
    glyphs = R.golden_glyphs(row, GET)
    if row['outcome'] == 'value_error':
        with pytest.raises(ValueError, match='read-only'):
            R.render_pixels(glyphs, row['boxes'], row['shape'], row['case'])
        assert 'read-only' in row['message']
        return
    got = R.render_pixels(glyphs, row['boxes'], row['shape'], row['case'])
    if row['outcome'] == 'none':
        assert got is None
        return
    assert R.same_bits(got['image'], GET(row['image'])) and R.same_bits(got['mask'], GET(row['mask']))
    assert (got['score'] is None) == (row['score'] is None)
    if got['score'] is not None:
        assert R.same_bits(got['score'], GET(row['score']))       # float32 as bit patterns
    assert got['boxes'] == row['char_boxes'] and got['interp'] == row['interp']


def plan_of(name):
    from vkit_amd.engine.font import plan_text_line
    case = R.case(name)
    run_config, font_face, render, enlarge, shrink = R.amd_arguments(case)
    rng = np.random.default_rng(case['seed'])
    return plan_text_line(run_config, font_face, render, rng, enlarge, shrink), rng


@pytest.mark.parametrize('name', list(R.CASES))
def test_host_planning_equals_the_golden(name):
    from vkit_amd.engine.font import estimate_font_size
    row = ROWS[name]
    if row['outcome'] == 'value_error':
        with pytest.raises(ValueError, match='read-only'):
            plan_of(name)
        return
    plan, rng = plan_of(name)
    assert rng.bit_generator.state == row['rng_state']
    if row['outcome'] == 'none':
        assert plan is None
        return
    assert list(plan.pasted) == row['shape'] and R.box_list(plan.pasted_char_boxes) == row['boxes']
    assert len(plan.char_glyphs) == len(row['glyphs'])
    for glyph, want in zip(plan.char_glyphs, row['glyphs']):
        assert R.same_bits(glyph.image.mat, GET(want['image']))
        assert (glyph.score_map is None) == (want['score'] is None)
        if glyph.score_map is not None:
            assert R.same_bits(glyph.score_map.mat, GET(want['score']))
        assert (glyph.char, glyph.ascent) == (want['char'], want['ascent'])
        assert [glyph.pad_up, glyph.pad_down, glyph.pad_left, glyph.pad_right] == want['pads']
        assert [glyph.ref_ascent_plus_pad_up, glyph.ref_char_height, glyph.ref_char_width] == want['ref']
    assert plan.out == tuple(GET(row['mask']).shape)
    assert R.box_list(plan.char_boxes) == row['char_boxes'] and [b.char for b in plan.char_boxes] == [g['char'] for g in row['glyphs']][:len(plan.char_boxes)]
    assert plan.cv_resize_interpolation == row['interp'] and plan.text == row['text'] and plan.is_hori == row['is_hori']
    assert estimate_font_size(plan.run_config) == row['font_size']
    # the plan names the same pixels as the restatement: resized shape, pad and clean-up
    case = row['case']
    target = case['height'] if case['hori'] else case['width']
    own = row['shape'][0] if case['hori'] else row['shape'][1]
    assert (plan.resized != plan.pasted) == (own / target < 0.8 or own > target)


def test_cases_hold_what_they_are_named_for():
    def plan(name):
        return plan_of(name)[0]
    one = plan('one_pixel_glyph')
    assert one.char_glyphs[0].image.shape == (1, 1) and len(plan('one_char').char_boxes) == 1
    boxes = R.box_list(plan('kerning_overlap').pasted_char_boxes)
    assert boxes[1][2] <= boxes[0][3]                                   # two char boxes overlap
    assert ' ' in plan('words').text
    for name in R.CASES:
        if name.startswith(('enlarge_', 'mono_enlarge')):
            p = plan(name)
            assert p.resized[0] > p.pasted[0] and p.pasted[0] / p.run_config.height < 0.8, name
        if name.startswith(('shrink_', 'mono_shrink')):
            p = plan(name)
            assert p.resized[0] < p.pasted[0], name
    p = plan('shrink_area_integer')
    assert p.pasted == (2 * p.resized[0], 2 * p.resized[1]) and p.cv_resize_interpolation == 3
    p = plan('shrink_area_fraction')
    assert p.pasted[0] % p.resized[0] or p.pasted[1] % p.resized[1]
    p = plan('shrink_linear_half')
    assert p.pasted[0] == 2 * p.resized[0] and p.cv_resize_interpolation == 5
    assert (plan('pad_even').run_config.height - plan('pad_even').pasted[0]) % 2 == 0 and plan('pad_even').resized == plan('pad_even').pasted
    assert (plan('pad_odd').run_config.height - plan('pad_odd').pasted[0]) % 2 == 1 and plan('pad_odd').pad_up == 1
    p = plan('trim_no_overlap')
    assert p.cleanup is None and len(p.char_boxes) < len(p.char_glyphs)
    p = plan('trim_cleanup')
    assert p.cleanup and p.resized == p.pasted and p.cleanup[1].shape == p.char_glyphs[p.cleanup[0]].image.shape
    for name in ('trim_cleanup_resized', 'trim_cleanup_shrunk', 'trim_cleanup_linear', 'lcd_enlarge_cleanup'):
        p = plan(name)
        assert p.cleanup and p.cleanup[1].shape != p.char_glyphs[p.cleanup[0]].image.shape, name
        assert p.cleanup[3].shape != p.char_glyphs[p.cleanup[2]].image.shape, name
    p = plan('trim_drop_last')                                           # the last box ends inside the width, the image does not
    assert len(p.char_boxes) == len(p.char_glyphs) - 1 and p.resized[1] > p.run_config.width
    last = p.pasted_char_boxes[-1].to_conducted_resized_char_box(p.pasted, resized_height=p.run_config.height)
    assert last.right < p.run_config.width
    assert plan('lcd_gamma_1').char_glyphs[0].image.mat.ndim == 3 and plan('lcd_gamma_2.2').run_config.style.glyph_color_gamma == 2.2
    assert set(np.unique(plan('mono_shrink').char_glyphs[0].image.mat)) <= {0, 255}
    p = plan('vert_resized')
    assert not p.is_hori and p.resized != p.pasted
    p = plan('vert_padded_lcd')
    assert not p.is_hori and p.pad_left > 0 and p.resized == p.pasted
    b0, b1 = p.pasted_char_boxes[0], p.char_boxes[0]
    assert (b1.left - b0.left, b1.right - b0.right) == (p.pad_left, p.run_config.width - p.pasted[1] - p.pad_left)
    p = plan('vert_trimmed')
    assert len(p.char_boxes) < len(p.char_glyphs) and p.cleanup is None
    # glyph features of the fake rasteriser: trimmed borders, negative bearings
    assert any(g['pads'][0] > 0 and g['pads'][2] > 0 for row in ROWS.values() for g in row['glyphs'])
    assert any(R.fake_glyph(c, 'default', 12)[0].bitmap_left < 0 for c in R.CHARS)


def test_lcd_value_at_gamma_1_is_the_numpy_expression_for_all_256_values():
    """The gamma-1 table the library's host code forms -- (uint8)((1.0 - v / 255.0) * 255.0) in IEEE double, restated here on
    Python floats -- equals the reference's numpy expression for every v.  Plain ``255 - v`` does NOT: 1 - v / 255.0 rounds and
    50 products fall just below the integer, so the kernel cannot take that shortcut."""
    from vkit_amd.engine.font import lcd_paste_plane
    v = np.arange(256, dtype=np.uint8)
    want = ((1 - np.power(v / 255.0, 1.0)) * 255).astype(np.uint8)
    assert lcd_paste_plane(v.reshape(16, 16), 1.0).reshape(-1).tobytes() == want.tobytes()
    device = np.array([int((1.0 - float(x) / 255.0) * 255.0) for x in range(256)], np.uint8)
    assert device.tobytes() == want.tobytes()
    differs = np.flatnonzero(want != 255 - v)
    assert len(differs) == 50 and differs[0] == 43 and (want[differs] == 254 - v[differs]).all()


def test_existing_containers_still_construct_with_their_old_keyword_sets():
    from vkit_amd.element import Box, Image, Mask, ScoreMap
    from vkit_amd.engine.font import CharBox, CharGlyph, TextLine
    glyph = CharGlyph(image=Image(mat=np.ones((3, 2), np.uint8)), score_map=ScoreMap(mat=np.ones((3, 2), np.float32)), ref_char_height=4,
                      ref_char_width=3)
    assert (glyph.char, glyph.ascent, glyph.pad_up, glyph.pad_down, glyph.pad_left, glyph.pad_right, glyph.ref_ascent_plus_pad_up) == ('', 0, 0, 0, 0, 0, 0)
    positional = CharGlyph(Image(mat=np.ones((3, 2), np.uint8)), None, 4, 3)
    assert (positional.ref_char_height, positional.ref_char_width) == (4, 3)
    box = Box(up=0, down=2, left=0, right=1)
    line = TextLine(image=Image(mat=np.zeros((3, 2, 3), np.uint8), box=box), mask=Mask(mat=np.ones((3, 2), np.uint8), box=box), score_map=None,
                    char_boxes=[CharBox(char='x', box=box)], char_glyphs=[glyph], cv_resize_interpolation=2, is_hori=True)
    assert line.glyph_color == (0, 0, 0) and not line.shifted
    assert (line.style, line.font_size, line.text, line.font_variant) == (None, 0, '', None)
    tinted = TextLine(image=line.image, mask=line.mask, score_map=None, char_boxes=line.char_boxes, char_glyphs=[glyph],
                      cv_resize_interpolation=2, is_hori=True, glyph_color=(1, 2, 3), shifted=True)
    assert tinted.glyph_color == (1, 2, 3) and tinted.box == box
    with pytest.raises(AssertionError):
        CharGlyph(image=glyph.image, score_map=None, ref_char_height=4, ref_char_width=3, pad_up=-1)


def test_render_char_glyphs_from_text_raises_as_the_reference_does():
    from vkit_amd.engine.font import render_char_glyphs_from_text
    case = R.case('words')
    run_config, font_face, render, _, _ = R.amd_arguments(case)
    # (the reference looks for leading spaces at index 0 only, where a space never reaches the check: they pass and count as a word space)
    assert render_char_glyphs_from_text(run_config, font_face, render, list(' ab'))[1] == [1, 0]
    with pytest.raises(RuntimeError, match='Trailing'):
        render_char_glyphs_from_text(run_config, font_face, render, list('ab '))
    glyphs, spaces = render_char_glyphs_from_text(run_config, font_face, render, list('a  b'))
    assert len(glyphs) == 2 and spaces == [0, 2]
