"""The page's symbol, barcode and frame layers against tests/golden/page_layers.npz (made by the reference's own steps and engines:
tests/golden/make_page_layers_golden.py).  No GPU: the numpy restatement (tests/page_layers_restate.py) equals every golden plane,
and the host ``plan`` of every step and engine equals the reference's records field for field and leaves the generator in the
reference's state; the device render is not touched."""
import numpy as np
import pytest
from numpy.random import default_rng

import page_layers_restate as R

INDEX, GET = R.golden()
TEXTURES = R.symbol_textures()


def ids(rows, key):
    return [key(r) for r in rows]


# ---- the restatement equals the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', INDEX['symbol_runs'], ids=lambda r: f"{r['name']}-{r['seed']}")
def test_symbol_restatement_equals_golden(run):
    for (up, left, h, w, alpha), row in zip(run['layout'], run['symbols']):
        src = TEXTURES[row['file']]
        if row['color'] is None:
            image, plane = R.symbol_rgba(src, (h, w), alpha)
        else:
            image, plane = R.symbol_gray(src, (h, w), alpha, row['color'])
        assert R.same_bits(image, GET(row['image']))
        assert R.same_bits(plane, GET(row['alpha']))


@pytest.mark.parametrize('run', INDEX['barcode_runs'], ids=lambda r: f"{r['kind']}-{r['shape'][0]}x{r['shape'][1]}-{r['seed']}")
def test_barcode_restatement_equals_golden(run):
    plane, _ = R.score(GET(run['mask']), tuple(run['shape']), run['alpha'])
    assert R.same_bits(plane, GET(run['score_map']))


def all_frames():
    return INDEX['frames'] + [f for r in INDEX['frame_runs'] for f in r['frames']]


def test_frame_restatement_equals_golden():
    for row in all_frames():
        assert R.same_bits(R.frame(row['box_shape'], row['thickness'], row['alpha'], row['trims']), GET(row['plane'])), row


def test_textures_are_the_stored_ones():
    data = np.load(R.os.path.join(R.HERE, 'golden', 'page_layers.npz'))
    for name, tex in TEXTURES.items():
        assert R.same_bits(tex, data['tex_' + name])


# ---- what keeps the goldens honest, on the stored data alone ---------------------------------------------------------------------
def test_clip_case_clips():
    clipped = 0
    for run in INDEX['barcode_runs']:
        _, raw = R.score(GET(run['mask']), tuple(run['shape']), run['alpha'])
        if raw is not None and run['alpha'] == 1.0:
            assert (raw > 1).any() and (raw < 0).any()
            assert GET(run['score_map']).max() == 1.0 and GET(run['score_map']).min() == 0.0
            clipped += 1
    assert clipped >= 1
    assert any(tuple(GET(r['mask']).shape) == tuple(r['shape']) for r in INDEX['barcode_runs'])      # no resize, no clip
    code39 = [r for r in INDEX['barcode_runs'] if r['kind'] == 'code39']
    assert code39 and all(tuple(GET(r['mask']).shape) != (40, 150) for r in code39)                  # the trim ran


def test_nan_case_is_all_nan():
    rows = [row for run in INDEX['symbol_runs'] for row in run['symbols'] if row['file'] == 'rgba_zero']
    assert rows and all(np.isnan(GET(row['alpha'])).all() for row in rows)
    others = [row for run in INDEX['symbol_runs'] for row in run['symbols'] if row['file'] != 'rgba_zero']
    assert not any(np.isnan(GET(row['alpha'])).any() for row in others)


def test_peak_case_has_its_maximum_on_one_pixel_of_the_last_tile():
    run = [r for r in INDEX['symbol_runs'] if r['name'].startswith('rgba_peak')][0]
    plane = GET(run['symbols'][0]['alpha'])
    ys, xs = np.nonzero(plane == plane.max())
    assert len(ys) == 1 and ys[0] // 4 == (plane.shape[0] - 1) // 4 and xs[0] // 64 == (plane.shape[1] - 1) // 64
    assert (plane.shape[0] + 3) // 4 * ((plane.shape[1] + 63) // 64) > 1


def test_sparse_gray_case_has_zeros_next_to_ink():
    run = [r for r in INDEX['symbol_runs'] if r['name'].startswith('gray_sparse')][0]
    plane = GET(run['symbols'][0]['alpha'])
    assert (plane == 0).any() and (plane > 0).any()


def test_all_four_colour_modes_occur():
    colours = [tuple(row['color']) for run in INDEX['symbol_runs'] for row in run['symbols'] if row['color'] is not None]
    assert any(c[0] == c[1] == c[2] for c in colours)
    for channel in range(3):
        assert any(c[channel] > 0 and sum(c) == c[channel] for c in colours)


def test_all_four_trims_occur_and_frames_are_mostly_non_empty():
    named = {r['name']: r for r in INDEX['frames']}
    assert [bool(t) for t in named['no_trim']['trims']] == [False] * 4
    for k, side in enumerate(('up', 'down', 'left', 'right')):
        assert [bool(t) for t in named['trim_' + side]['trims']] == [i == k for i in range(4)]
    assert all(named['trim_all']['trims'])
    assert named['thin']['thickness'] == 1
    assert not GET(named['interior_only']['plane']).any()
    seeded = [f for r in INDEX['frame_runs'] for f in r['frames']]
    assert len(seeded) >= 40
    assert sum(bool(GET(f['plane']).any()) for f in seeded) >= 0.9 * len(seeded)


# ---- the host plans equal the reference ------------------------------------------------------------------------------------------
def layout_of(**fields):
    from vkit_amd.pipeline.text_detection import PageLayout, PageLayoutStepOutput
    return PageLayoutStepOutput(page_layout=PageLayout(**fields))


def box_of(up, left, h, w):
    from vkit_amd.element import Box
    return Box(up=up, down=up + h - 1, left=left, right=left + w - 1)


@pytest.mark.parametrize('run', INDEX['symbol_runs'], ids=lambda r: f"{r['name']}-{r['seed']}")
def test_symbol_plan_equals_the_reference(run):
    from vkit_amd.pipeline import text_detection as T
    step = T.PageNonTextSymbolStep(T.PageNonTextSymbolStepConfig(symbol_image_folders=[], **run['overrides']),
                                   selector=R.FakeSelector(TEXTURES, [f + '.png' for f in run['files']]))
    symbols = [T.LayoutNonTextSymbol(box=box_of(up, left, h, w), alpha=alpha) for up, left, h, w, alpha in run['layout']]
    rng = default_rng(run['seed'])
    plans = step.plan(T.PageNonTextSymbolStepInput(page_layout_step_output=layout_of(height=160, width=200, layout_non_text_symbols=symbols)), rng)
    assert rng.bit_generator.state == run['rng_state']
    assert len(plans) == len(run['symbols'])
    for plan, row, symbol in zip(plans, run['symbols'], symbols):
        assert plan.image_file == row['file'] + '.png'
        assert (None if plan.symbol_color is None else list(plan.symbol_color)) == row['color']
        assert plan.box == symbol.box and plan.alpha == symbol.alpha


def test_symbol_plan_refuses_a_three_channel_file():
    from vkit_amd.pipeline import text_detection as T
    step = T.PageNonTextSymbolStep(T.PageNonTextSymbolStepConfig(symbol_image_folders=[]), selector=R.FakeSelector(TEXTURES, ['rgb_3ch.png']))
    symbols = [T.LayoutNonTextSymbol(box=box_of(0, 0, 4, 4), alpha=0.5)]
    with pytest.raises(NotImplementedError):
        step.plan(T.PageNonTextSymbolStepInput(page_layout_step_output=layout_of(height=8, width=8, layout_non_text_symbols=symbols)),
                  default_rng(0))


def make_barcode_engine(kind, overrides):
    from vkit_amd.engine import barcode as B
    if kind == 'qr':
        return B.BarcodeQrEngine(B.BarcodeQrEngineInitConfig(**overrides), func_encode=R.qr_image)
    return B.BarcodeCode39Engine(B.BarcodeCode39EngineInitConfig(**overrides), func_encode=R.code39_image)


@pytest.mark.parametrize('run', INDEX['barcode_runs'], ids=lambda r: f"{r['kind']}-{r['shape'][0]}x{r['shape'][1]}-{r['seed']}")
def test_barcode_plan_equals_the_reference(run):
    from vkit_amd.engine.barcode import BarcodeEngineRunConfig
    engine = make_barcode_engine(run['kind'], run['overrides'])
    rng = default_rng(run['seed'])
    plan = engine.plan(BarcodeEngineRunConfig(height=run['shape'][0], width=run['shape'][1]), rng)
    assert rng.bit_generator.state == run['rng_state']
    assert plan.text == run['text'] and plan.alpha == run['alpha'] and (plan.height, plan.width) == tuple(run['shape'])
    assert R.same_bits(plan.mask, GET(run['mask']))


def test_barcode_page_plan_equals_the_reference():
    from vkit_amd.pipeline import text_detection as T
    page = R.BARCODE_PAGE
    step = T.PageBarcodeStep(T.PageBarcodeStepConfig(), func_encode_qr=R.qr_image, func_encode_code39=R.code39_image)
    rng = default_rng(page['seed'])
    plan = step.plan(T.PageBarcodeStepInput(page_layout_step_output=layout_of(
        height=page['shape'][0], width=page['shape'][1], layout_barcode_qrs=[T.LayoutBarcodeQr(box=box_of(*b)) for b in page['qrs']],
        layout_barcode_code39s=[T.LayoutBarcodeCode39(box=box_of(*b)) for b in page['code39s']])), rng)
    assert rng.bit_generator.state == INDEX['barcode_page']['rng_state']
    assert [p.text for _, p in plan.qrs + plan.code39s] == INDEX['barcode_page']['texts']
    for (_, p), entry in zip(plan.qrs + plan.code39s, INDEX['barcode_page']['qrs'] + INDEX['barcode_page']['code39s']):
        assert R.same_bits(R.score(p.mask, (p.height, p.width), p.alpha)[0], GET(entry))


def test_code39_trim_asserts_like_the_reference():
    from vkit_amd.engine.barcode import BarcodeCode39Engine
    with pytest.raises(AssertionError):
        BarcodeCode39Engine.convert_barcode_image_to_mask(np.full((8, 8), 255, np.uint8))
    one_column = np.full((8, 8), 255, np.uint8)
    one_column[2:6, 3] = 0
    with pytest.raises(AssertionError):
        BarcodeCode39Engine.convert_barcode_image_to_mask(one_column)


def test_default_encoders_name_the_missing_library():
    from vkit_amd.engine.barcode import code39, qr
    for module, func, words in ((qr, qr.default_qr_encode, 'cv2'), (code39, code39.default_code39_encode, 'python-barcode')):
        try:
            func('abc')
        except RuntimeError as exc:
            assert words in str(exc)


def frame_plan_row(plan):
    box = plan.page_box
    return dict(thickness=plan.border_thickness, alpha=plan.alpha, box_shape=[plan.box_height, plan.box_width], trims=list(plan.trims),
                page_box=[box.up, box.down, box.left, box.right], color=list(plan.color))


@pytest.mark.parametrize('row', INDEX['frames'], ids=lambda r: r['name'])
def test_frame_plan_equals_the_reference(row):
    from vkit_amd.element import Box
    from vkit_amd.pipeline import text_detection as T
    step = T.PageTextLineBoundingBoxStep(T.PageTextLineBoundingBoxStepConfig(**row['overrides']))
    rng = default_rng(row['seed'])
    plan = step.plan_text_line_bounding_box(row['page'][0], row['page'][1], R.text_line_of(row['line_box'], row['ref_heights'], row['color'], Box),
                                            rng)
    assert rng.bit_generator.state == row['rng_state']
    assert frame_plan_row(plan) == {k: row[k] for k in frame_plan_row(plan)}


@pytest.mark.parametrize('run', INDEX['frame_runs'], ids=lambda r: str(r['seed']))
def test_frame_page_plan_equals_the_reference(run):
    from vkit_amd.element import Box
    from vkit_amd.pipeline import text_detection as T
    lines = R.frame_run_lines(run['seed'])
    step = T.PageTextLineBoundingBoxStep(T.PageTextLineBoundingBoxStepConfig(**R.FRAME_RUN_CONFIG))
    collection = T.PageTextLineCollection(height=160, width=220, text_lines=[R.text_line_of(b, hs, c, Box) for b, hs, c, _ in lines],
                                          short_text_line_flags=[short for _, _, _, short in lines])
    rng = default_rng(run['seed'])
    plans = step.plan(T.PageTextLineBoundingBoxStepInput(page_text_line_step_output=T.PageTextLineStepOutput(
        page_text_line_collection=collection,
        page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=160, width=220))), rng)
    assert rng.bit_generator.state == run['rng_state']
    assert [frame_plan_row(p) for p in plans] == [{k: row[k] for k in frame_plan_row(p)} for p, row in zip(plans, run['frames'])]
    assert len(plans) == len(run['frames'])


def test_frame_asserts_like_the_reference():
    from vkit_amd.element import Box
    from vkit_amd.pipeline import text_detection as T
    # a ring as thick as half the box leaves no interior of two rows: the reference's first assert
    step = T.PageTextLineBoundingBoxStep(T.PageTextLineBoundingBoxStepConfig(offset_ratio_min=0.0, offset_ratio_max=0.0,
                                                                             border_thickness_ratio_min=1.0, border_thickness_ratio_max=1.0))
    with pytest.raises(AssertionError):
        step.plan_text_line_bounding_box(100, 100, R.text_line_of((10, 19, 10, 59), [10], (0, 0, 0), Box), default_rng(0))


def test_page_layout_grows_additively():
    from vkit_amd.pipeline import text_detection as T
    layout = T.PageLayout(height=3, width=4)
    assert (layout.layout_images, layout.layout_barcode_qrs, layout.layout_barcode_code39s, layout.layout_non_text_symbols) == ((), (), (), ())


def test_record_table_matches_the_header():
    from vkit_amd import _native
    import re
    header = open(R.os.path.join(R.os.path.dirname(R.HERE), 'include', 'vkx.h')).read()
    body = re.search(r'typedef struct vkx_page_layer \{(.*?)\} vkx_page_layer;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip(' *').split('[')[0] for decl in body.split(';') if decl.strip()
             for n in decl.strip().split(None, 1)[1].replace('void *', '').replace('const ', '').split(',')]
    assert names == list(_native.PAGE_LAYER_DTYPE.names)
    assert 'vkx_page_layers_dev' in _native.EXPORTED_SYMBOLS
