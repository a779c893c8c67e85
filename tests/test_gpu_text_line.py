"""vkit_amd.engine.font's text-line half on the GPU (csrc/text_line.hip): render_text_line_meta against the goldens of the
reference's own function and against the numpy restatement, with host and resident outputs; None and the ValueError where the
reference has them, nothing launched; a batch against single calls; the launch and synchronisation budget; the C entry point's
refusals; and rendered lines through PageAssemblerStep and fill_text_line_to_seal_impression.  Every comparison is exact
(float32 as bit patterns)."""
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seal_impression_restate as SR  # noqa: E402
import text_line_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

INDEX, GET = R.golden()
ROWS = {row['name']: row for row in INDEX['cases']}
RENDERABLE = [name for name, case in R.CASES.items() if case['expect'] == 'line']
_restated = {}


def restated(name):
    """the restatement of a golden case on the golden's glyphs and placement, computed once"""
    if name not in _restated:
        row = ROWS[name]
        _restated[name] = R.render_pixels(R.golden_glyphs(row, GET), row['boxes'], row['shape'], row['case'])
    return _restated[name]


def render(case, rng=None):
    from vkit_amd.engine.font import render_text_line_meta
    run_config, font_face, func, enlarge, shrink = R.amd_arguments(case)
    rng = rng or np.random.default_rng(case['seed'])
    return render_text_line_meta(run_config, font_face, func, rng, enlarge, shrink), rng


def planes(line):
    return line.image.mat, line.mask.mat, None if line.score_map is None else line.score_map.mat


def same_planes(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and R.same_bits(x, y)) for x, y in zip(a, b))


def restated_case(case):
    """the restatement of any case: the package's plan for the placement, the restatement for every pixel"""
    from vkit_amd.engine.font import plan_text_line
    run_config, font_face, func, enlarge, shrink = R.amd_arguments(case)
    plan = plan_text_line(run_config, font_face, func, np.random.default_rng(case['seed']), enlarge, shrink)
    if plan is None:
        return None
    data = [dict(image=g.image.mat, score=None if g.score_map is None else g.score_map.mat) for g in plan.char_glyphs]
    return R.render_pixels(data, R.box_list(plan.pasted_char_boxes), plan.pasted, case)


# ---- the public function ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', (False, True), ids=('host', 'resident'))
@pytest.mark.parametrize('name', RENDERABLE)
def test_single_call_equals_golden_and_restatement(name, resident):
    from vkit_amd import _native as N
    row, case = ROWS[name], R.case(name)
    with N.resident(resident):
        line, rng = render(case)
    assert line.image.on_device == resident and line.mask.on_device == resident
    got = planes(line)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.uint8 and (got[2] is None or got[2].dtype == np.float32)
    assert same_planes(got, (GET(row['image']), GET(row['mask']), GET(row['score'])))
    want = restated(name)
    assert same_planes(got, (want['image'], want['mask'], want['score']))
    assert R.box_list(line.char_boxes) == row['char_boxes'] and line.cv_resize_interpolation == row['interp']
    assert (line.text, line.font_size, line.is_hori, len(line.char_glyphs)) == (row['text'], row['font_size'], row['is_hori'], row['n_glyphs'])
    assert list(line.glyph_color) == row['glyph_color'] and line.style is not None and line.font_variant is None
    assert line.box.shape == got[1].shape and line.image.box == line.box and (line.score_map is None or line.score_map.box == line.box)
    assert rng.bit_generator.state == row['rng_state']


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
            try:
                out = call()
            except ValueError as error:
                out = error
            n_syncs = len(syncs)
            timings = ctx.timings()
        finally:
            ctx.set_timing(0)
    return out, {name: cnt for name, (_ms, cnt) in timings.items()}, n_syncs


def test_none_and_value_error_arise_where_the_reference_has_them_with_nothing_launched(monkeypatch):
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    for name, case in R.CASES.items():
        if case['expect'] == 'line':
            continue
        out, launches, _ = _count(monkeypatch, ctx, lambda: render(R.case(name)))
        assert launches == {}, name
        if case['expect'] == 'none':
            assert out[0] is None and out[1].bit_generator.state == ROWS[name]['rng_state'], name
        else:
            assert isinstance(out, ValueError) and 'read-only' in str(out), name


def test_lcd_glyph_with_all_256_values_pastes_the_numpy_expression():
    """gamma 1: what the kernel pastes equals ((1 - v / 255.0) * 255).astype(uint8) for every value (which is not 255 - v)"""
    from vkit_amd import _native as N
    glyph = np.arange(256, dtype=np.uint8).reshape(16, 16)
    glyph = np.stack([glyph, glyph[::-1], glyph.T], axis=2)
    ink = np.any(glyph > 0, axis=2)
    chars = np.zeros(1, N.TEXT_CHAR_DTYPE)
    chars[0]['score_off'] = chars[0]['paste_off'] = -1
    chars[0]['glyph_h'] = chars[0]['glyph_w'] = 16
    lines = np.zeros(1, N.TEXT_LINE_DTYPE)
    line = lines[0]
    line['channels'], line['paste_h'], line['paste_w'], line['resized_h'], line['resized_w'] = 3, 16, 16, 16, 16
    line['interpolation'], line['out_h'], line['out_w'], line['score_off'], line['mask_off'] = 2, 16, 16, -1, 768
    dst = N.default_ctx().dev_empty((1024,), np.uint8)
    N.text_lines(chars, lines, glyph.reshape(-1), dst)
    host = np.array(dst.host())
    want = np.full((16, 16, 3), 255, np.uint8)
    want[ink] = ((1 - np.power(glyph / 255.0, 1.0)) * 255).astype(np.uint8)[ink]
    assert host[:768].tobytes() == want.tobytes() and host[768:].tobytes() == ink.astype(np.uint8).tobytes()
    assert (want[ink] != 255 - glyph[ink]).any()


def test_line_of_more_chars_than_a_workgroup_holds_at_a_time():
    """80 chars: the char records go through LDS in two rounds"""
    case = R._case('ab' * 40, 12, 160, 6, seed=5)
    line, _ = render(case)
    want = restated_case(case)
    assert len(line.char_glyphs) < 80 and same_planes(planes(line), (want['image'], want['mask'], want['score']))
    wide = dict(case, width=2000)
    line, _ = render(wide)
    want = restated_case(wide)
    assert len(line.char_glyphs) == 80 and same_planes(planes(line), (want['image'], want['mask'], want['score']))


# ---- the batch ---------------------------------------------------------------------------------------------------
def batch_cases():
    return [(name, R.case(name)) for name in R.CASES] + R.random_cases()


def add_all(batch, cases):
    handles = []
    for name, case in cases:
        run_config, font_face, func, enlarge, shrink = R.amd_arguments(case)
        rng = np.random.default_rng(case['seed'])
        try:
            handles.append((name, case, batch.add(run_config, font_face, func, rng, enlarge, shrink), rng))
        except ValueError:
            handles.append((name, case, ValueError, rng))
    return handles


def test_batch_equals_single_calls():
    """every case and 30 random small lines in one call: each line has the bits of its single call"""
    from vkit_amd.engine.font import TextLineBatch
    batch = TextLineBatch()
    handles = add_all(batch, batch_cases())
    lines = batch.render()
    assert len(lines) == sum(1 for _, _, h, _ in handles if h is not None and h is not ValueError) >= len(RENDERABLE) + 20
    assert batch.render() == []
    kinds = set()
    for name, case, handle, rng in handles:
        if handle is ValueError:
            assert case['expect'] == 'value_error' or not case['hori'], name
            continue
        single, single_rng = render(case)
        assert rng.bit_generator.state == single_rng.bit_generator.state, name
        if handle is None:
            assert single is None, name
            continue
        line = handle.text_line
        assert same_planes(planes(line), planes(single)), name
        assert R.box_list(line.char_boxes) == R.box_list(single.char_boxes) and line.text == single.text, name
        kinds.add((case['kind'], case['hori'], handle.plan.resized != handle.plan.pasted))
        if name in ROWS:
            assert same_planes(planes(line), (GET(ROWS[name]['image']), GET(ROWS[name]['mask']), GET(ROWS[name]['score']))), name
        else:
            want = restated_case(case)
            assert same_planes(planes(line), (want['image'], want['mask'], want['score'])), name
    # every glyph kind, both directions, resized and not
    assert {k[0] for k in kinds} == {'default', 'lcd', 'mono'} and {k[1:] for k in kinds} == {(True, True), (True, False), (False, True), (False, False)}, kinds


def test_launch_and_sync_budget(monkeypatch):
    """one line and 70 lines: the same launches, at most three, no synchronisation"""
    from vkit_amd import _native as N
    from vkit_amd.engine.font import TextLineBatch
    ctx = N.default_ctx()
    seen = []
    with N.resident(True):
        for cases in ([('one_char', R.case('one_char'))], batch_cases() + [(n, R.case(n)) for n in RENDERABLE[:12]]):
            def run():
                batch = TextLineBatch()
                add_all(batch, cases)
                return batch.render()
            run()                                               # warm the scratch slots
            lines, launches, syncs = _count(monkeypatch, ctx, run)
            seen.append((launches, syncs))
            assert len(lines) == 1 or len(lines) >= 70
            for line in lines[:3]:
                assert line.image.on_device and line.mask.on_device
    assert seen[0] == seen[1] == ({'k_text_paste': 1, 'k_text_resize': 1}, 0), seen
    assert sum(seen[0][0].values()) <= 3


# ---- the C entry point -----------------------------------------------------------------------------------------
def tables(names):
    from vkit_amd.engine.font import build_text_line_tables, plan_text_line
    plans = []
    for name in names:
        case = R.case(name)
        run_config, font_face, func, enlarge, shrink = R.amd_arguments(case)
        plans.append(plan_text_line(run_config, font_face, func, np.random.default_rng(case['seed']), enlarge, shrink))
    return build_text_line_tables(plans)


def raw_call(ctx, chars, lines, blob, dst, n_chars=None, n_lines=None, dst_bytes=None, chars_ptr=True, lines_ptr=True, blob_ptr=True,
             blob_bytes=None):
    from vkit_amd import _native as N
    blob = np.ascontiguousarray(blob, np.uint8)
    return N.lib().vkx_text_lines_dev(
        ctx.handle, chars.ctypes.data if chars_ptr else None, len(chars) if n_chars is None else n_chars,
        lines.ctypes.data if lines_ptr else None, len(lines) if n_lines is None else n_lines, blob.ctypes.data if blob_ptr else None,
        blob.size if blob_bytes is None else blob_bytes, c_void_p(dst.ptr) if dst is not None else None,
        dst.nbytes if dst_bytes is None else dst_bytes)


def test_lines_at_the_borders_of_the_64_x_4_tiles():
    """one raw call with an unresized line of 65 x 5 pixels (two tiles a row, two rows of tiles) and a line resized CUBIC from a
    32 x 2 pasted plane to 64 x 4 (exactly one tile), glyphs in the last rows and columns of both: the restatement's bits"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    rng = np.random.default_rng(65)
    color = (10, 200, 30)
    # (pasted shape, output shape, the glyph boxes [up, down, left, right] in the pasted plane)
    layout = (((5, 65), (5, 65), ([0, 4, 0, 29], [1, 4, 55, 64])), ((2, 32), (4, 64), ([0, 1, 0, 14], [1, 1, 16, 31])))
    chars, lines, parts, wants = [], np.zeros(2, N.TEXT_LINE_DTYPE), [], []
    blob_bytes = dst_bytes = 0
    for k, (pasted, out, boxes) in enumerate(layout):
        glyphs = []
        for up, down, left, right in boxes:
            score = (R.blocky(rng, (down - up + 1, right - left + 1), 1, 1, 5) / np.float32(4)).astype(np.float32)
            glyphs.append(dict(image=(score * 255).astype(np.uint8), score=score))
            record = np.zeros((), N.TEXT_CHAR_DTYPE)
            record['glyph_h'], record['glyph_w'], record['line'], record['up'], record['left'] = score.shape[0], score.shape[1], k, up, left
            record['image_off'], record['score_off'], record['paste_off'] = blob_bytes + score.size * 4, blob_bytes, -1
            parts += [score.view(np.uint8).reshape(-1), glyphs[-1]['image'].reshape(-1), np.zeros(-score.size % 4, np.uint8)]
            blob_bytes += sum(p.size for p in parts[-3:])
            chars.append(record)
        area = out[0] * out[1]
        line = lines[k]
        line['channels'], line['color'], line['has_score'], line['interpolation'] = 1, color, 1, R.INTERPOLATIONS['CUBIC']
        line['paste_h'], line['paste_w'], line['resized_h'], line['resized_w'], line['out_h'], line['out_w'] = pasted + out + out
        line['score_off'], line['image_off'], line['mask_off'] = dst_bytes, dst_bytes + 4 * area, dst_bytes + 7 * area
        dst_bytes += 8 * area
        case = dict(style=dict(glyph_color=color), hori=True, height=out[0], width=out[1], enlarge=R.INTERPOLATIONS['CUBIC'],
                    shrink=R.INTERPOLATIONS['AREA'])
        wants.append(R.render_pixels(glyphs, boxes, pasted, case))
        assert wants[-1]['mask'].shape == out and wants[-1]['interp'] == R.INTERPOLATIONS['CUBIC']
        assert wants[-1]['mask'][-1, -1] == 1 and wants[-1]['score'][-1, -1] > 0                    # ink in the last row and column
    assert (int(lines[1]['resized_h']), int(lines[1]['resized_w'])) != (int(lines[1]['paste_h']), int(lines[1]['paste_w']))
    dst = ctx.to_device(np.full(dst_bytes, 123, np.uint8))
    assert raw_call(ctx, np.array(chars, N.TEXT_CHAR_DTYPE), lines, np.concatenate(parts), dst) == 0
    got = np.array(dst.host())
    for line, want in zip(lines, wants):
        h, w = want['mask'].shape
        image = got[int(line['image_off']):int(line['image_off']) + 3 * h * w].reshape(h, w, 3)
        mask = got[int(line['mask_off']):int(line['mask_off']) + h * w].reshape(h, w)
        score = got[int(line['score_off']):int(line['score_off']) + 4 * h * w].view(np.float32).reshape(h, w)
        assert same_planes((image, mask, score), (want['image'], want['mask'], want['score'])), (h, w)


def test_abi_refusals():
    """every refusal of include/vkx.h: VKX_ERR_INVALID and nothing written; the unchanged tables still run and match"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    names = ('words', 'enlarge_cubic', 'trim_cleanup_resized', 'lcd_gamma_2.2', 'shrink_area_fraction', 'trim_cleanup')
    chars, lines, blob, nbytes = tables(names)
    sentinel = np.full(nbytes, 123, np.uint8)
    dst = ctx.to_device(sentinel)
    INVALID = -1

    def _download(arr):
        out = np.empty(arr.shape, arr.dtype)
        ctx.download(arr.ptr, out)
        return out

    def refused(c=chars, s=lines, b=blob, d=dst, **kw):
        rc = raw_call(ctx, c, s, b, d, **kw)
        ctx.sync()
        return rc == INVALID and _download(dst).tobytes() == sentinel.tobytes()

    def with_char(k=0, **over):
        c = chars.copy()
        for key, value in over.items():
            c[k][key] = value
        return c

    def with_line(k=0, **over):
        s = lines.copy()
        for key, value in over.items():
            s[k][key] = value
        return s

    first = {k: int(np.flatnonzero(chars['line'] == k)[0]) for k in range(len(lines))}
    assert refused(chars_ptr=False) and refused(lines_ptr=False) and refused(blob_ptr=False) and refused(d=None, dst_bytes=nbytes)
    assert refused(n_chars=0) and refused(n_chars=65537) and refused(n_lines=0) and refused(n_lines=4097)
    # a box outside its line
    assert refused(c=with_char(up=-1)) and refused(c=with_char(left=-1))
    assert refused(c=with_char(up=int(lines[0]['paste_h']) - int(chars[0]['glyph_h']) + 1))
    assert refused(c=with_char(left=int(lines[0]['paste_w']) - int(chars[0]['glyph_w']) + 1))
    assert refused(c=with_char(glyph_h=0)) and refused(c=with_char(glyph_w=32768))
    assert refused(c=with_char(line=len(lines))) and refused(c=with_char(line=-1)) and refused(c=with_char(first[1], line=3))
    # a destination outside dst, misaligned, or overlapping another
    assert refused(s=with_line(1, image_off=nbytes - 1)) and refused(s=with_line(1, mask_off=-1)) and refused(s=with_line(0, score_off=nbytes - 4))
    assert refused(s=with_line(0, score_off=int(lines[0]['score_off']) + 2)) and refused(dst_bytes=nbytes - 1)
    assert refused(s=with_line(1, image_off=int(lines[0]['image_off']))) and refused(s=with_line(1, mask_off=int(lines[0]['score_off']) + 8))
    # a blob offset out of range
    assert refused(c=with_char(image_off=blob.size)) and refused(c=with_char(image_off=-1)) and refused(c=with_char(score_off=blob.size - 4))
    assert refused(c=with_char(score_off=int(chars[0]['score_off']) + 2)) and refused(c=with_char(score_off=-1))
    lcd = first[3]
    assert int(chars[lcd]['paste_off']) >= 0 and refused(c=with_char(lcd, paste_off=blob.size - 3)) and refused(c=with_char(0, paste_off=0))
    assert refused(blob_bytes=int(chars['image_off'].max()))
    # an unknown interpolation (the plain NEAREST and LINEAR are not among the five a text line samples)
    for code in (7, -1, 0, 1):
        assert refused(s=with_line(1, interpolation=code)), code
    # an AREA enlargement: of a line, and of a clean-up glyph
    assert lines[1]['resized_h'] > lines[1]['paste_h'] and refused(s=with_line(1, interpolation=3))
    assert lines[2]['cleanup'] == 1 and refused(s=with_line(2, interpolation=3))
    grown = [int(v) for v in lines[5]['trimmed_box']]
    grown[2] += 1
    assert lines[5]['cleanup'] == 1 and (lines[5]['resized_h'], lines[5]['resized_w']) == (lines[5]['paste_h'], lines[5]['paste_w'])
    assert refused(s=with_line(5, interpolation=3, trimmed_box=grown)) and not refused(s=with_line(5, interpolation=3))
    ctx.upload(dst.ptr, sentinel)             # (AREA with nothing to resize ran: back to the sentinel)
    # sides, pads, colours, channels, clean-up chars and boxes
    for field in ('paste_h', 'paste_w', 'resized_h', 'resized_w', 'out_h', 'out_w'):
        assert refused(s=with_line(1, **{field: 0})) and refused(s=with_line(1, **{field: 32768})), field
    assert refused(s=with_line(pad_up=-1)) and refused(s=with_line(pad_left=-1)) and refused(s=with_line(color=[0, 256, 0]))
    assert refused(s=with_line(channels=2)) and refused(s=with_line(has_score=0)) and refused(s=with_line(3, has_score=1))
    n2 = int((chars['line'] == 2).sum())
    assert refused(s=with_line(2, trimmed_char=n2)) and refused(s=with_line(2, kept_char=-1))
    assert refused(s=with_line(2, kept_box=[0, 0, int(lines[2]['out_h']) + 1, 1])) and refused(s=with_line(2, trimmed_box=[0, 0, 0, 1]))
    # and the unchanged tables still run, and match the public calls
    assert raw_call(ctx, chars, lines, blob, dst) == 0
    ctx.sync()
    got = _download(dst)
    for name, line in zip(names, lines):
        h, w = int(line['out_h']), int(line['out_w'])
        want = restated(name)
        assert got[int(line['image_off']):int(line['image_off']) + 3 * h * w].tobytes() == want['image'].tobytes(), name
        assert got[int(line['mask_off']):int(line['mask_off']) + h * w].tobytes() == want['mask'].tobytes(), name
        if want['score'] is not None:
            assert got[int(line['score_off']):int(line['score_off']) + 4 * h * w].tobytes() == want['score'].tobytes(), name


# ---- downstream: PageAssemblerStep and the seal engine ----------------------------------------------------------------
def restated_line(name, line):
    """the TextLine of a golden case with the restatement's planes and the rendered line's glyphs"""
    from vkit_amd.element import Box, Image, Mask, ScoreMap
    from vkit_amd.engine.font import CharBox, TextLine
    want = restated(name)
    box = Box.from_shape(want['mask'].shape)
    return TextLine(image=Image(mat=want['image'].copy(), box=box), mask=Mask(mat=want['mask'].copy(), box=box),
                    score_map=None if want['score'] is None else ScoreMap(mat=want['score'].copy(), box=box),
                    char_boxes=[CharBox(char=g.char, box=Box(up=b[0], down=b[1], left=b[2], right=b[3])) for g, b in zip(line.char_glyphs, want['boxes'])],
                    char_glyphs=line.char_glyphs, cv_resize_interpolation=want['interp'], is_hori=True,
                    glyph_color=tuple(line.glyph_color))


def test_rendered_lines_go_through_the_page_assembler_unchanged():
    """a 96 x 128 page with a default line (score-map composite) and an LCD line (mask composite): the page of the rendered lines
    equals the page of the same lines built by the restatement"""
    from numpy.random import default_rng
    from vkit_amd.element import Image
    from vkit_amd.pipeline.text_detection import page_assembler as T
    h, w = 96, 128
    placed = (('words', 10, 8), ('lcd_gamma_2.2', 40, 20), ('trim_cleanup_resized', 70, 60))

    def page_of(lines):
        rng = np.random.default_rng(5)
        background = Image(mat=SR.blocky(rng, (h, w), 8, 0, 16, np.uint8)[:, :, None].repeat(3, axis=2) * np.uint8(15))
        step_input = T.PageAssemblerStepInput(
            page_layout_step_output=T.PageLayoutStepOutput(T.PageLayout(height=h, width=w)),
            page_background_step_output=T.PageBackgroundStepOutput(background),
            page_image_step_output=T.PageImageStepOutput(page_image_collection=T.PageImageCollection(height=h, width=w),
                                                         page_bottom_layer_image=Image(mat=np.zeros((h, w, 3), np.uint8))),
            page_barcode_step_output=T.PageBarcodeStepOutput(height=h, width=w),
            page_text_line_step_output=T.PageTextLineStepOutput(
                page_text_line_collection=T.PageTextLineCollection(height=h, width=w, text_lines=lines, short_text_line_flags=[False] * len(lines)),
                page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=h, width=w)),
            page_non_text_symbol_step_output=T.PageNonTextSymbolStepOutput(),
            page_text_line_bounding_box_step_output=T.PageTextLineBoundingBoxStepOutput(),
            page_text_line_label_step_output=T.PageTextLineLabelStepOutput(
                page_char_polygon_collection=T.PageCharPolygonCollection(height=h, width=w),
                page_text_line_polygon_collection=T.PageTextLinePolygonCollection(height=h, width=w)))
        page = T.page_assembler_step_factory.create().run(step_input, default_rng(0)).page
        return page.image.mat, background.mat

    new, old = [], []
    for name, up, left in placed:
        line, _ = render(R.case(name))
        new.append(line.to_shifted_text_line(offset_y=up, offset_x=left))
        old.append(restated_line(name, line).to_shifted_text_line(offset_y=up, offset_x=left))
    new_page, background = page_of(new)
    old_page, _ = page_of(old)
    assert new_page.tobytes() == old_page.tobytes() and new_page.tobytes() != background.tobytes()


def test_rendered_line_goes_through_the_seal_engine_unchanged():
    """a 128 x 160 seal whose curved text line and internal text line are rendered lines: the filled score map and the char polygons
    equal those of the same lines built by the restatement"""
    from vkit_amd.element import Box, Mask, Point
    from vkit_amd.engine.seal_impression import CharSlot, SealImpression, TextLineSlot, fill_text_line_to_seal_impression
    curved, _ = render(R.case('enlarge_cubic'))
    internal, _ = render(R.case('words'))
    h, w = 128, 160
    ih, iw = internal.box.shape
    assert ih + 4 <= h and iw + 4 <= w

    def seal():
        slots = SR.ring_slots(np.random.default_rng(3), (h, w), len(curved.char_boxes), curved.box.height, reach=0.5)
        return SealImpression(alpha=0.7, color=(200, 0, 0), background_mask=Mask(mat=np.zeros((h, w), np.uint8)),
                              text_line_slots=[TextLineSlot(text_line_height=curved.box.height, char_aspect_ratio=0.8,
                                                            char_slots=[CharSlot(angle=c[0], point_up=Point.create(y=c[1], x=c[2]),
                                                                                 point_down=Point.create(y=c[3], x=c[4])) for c in slots])],
                              internal_text_line_box=Box(up=2, down=2 + ih - 1, left=2, right=2 + iw - 1))

    def xy(polygons):
        return [np.array([(p.smooth_x, p.smooth_y) for p in polygon.points], np.float64).tobytes() for polygon in polygons]

    new_map, new_polygons = fill_text_line_to_seal_impression(seal(), [0], [curved], internal)
    old_map, old_polygons = fill_text_line_to_seal_impression(seal(), [0], [restated_line('enlarge_cubic', curved)], restated_line('words', internal))
    assert SR.same_bits(new_map.mat, old_map.mat) and np.nanmax(new_map.mat) > 0
    assert xy(new_polygons) == xy(old_polygons) and len(new_polygons) > len(internal.char_boxes)
