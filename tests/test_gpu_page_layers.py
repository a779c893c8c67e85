"""GPU: the page's symbol, barcode and frame layers (csrc/page_layers.hip) through the public steps and engines against the
reference's outputs (tests/golden/page_layers.npz) and the numpy restatement (tests/page_layers_restate.py), in host and in
resident mode; the launch and synchronisation budget; the refusals of the C entry point; a page assembled from golden planes, from
the steps in host mode and from the steps in resident mode; a seeded random loop.  uint8 planes are compared exactly, float32 planes
under == with equal NaN positions."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_layers_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

INDEX, GET = R.golden()
TEXTURES = R.symbol_textures()


@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    """the symbol textures as PNG files (the real selector decodes and caches them), and a folder of RGB pictures"""
    from PIL import Image as PilImage
    root = tmp_path_factory.mktemp('page_layers')
    symbols, pictures = root / 'symbols', root / 'pictures'
    symbols.mkdir()
    pictures.mkdir()
    for name, tex in TEXTURES.items():
        PilImage.fromarray(tex).save(str(symbols / (name + '.png')))
    rng = default_rng(7)
    for k in range(3):
        PilImage.fromarray(R.blocky(rng, (90, 120), 6, 0, 256)[:, :, None].repeat(3, axis=2) ^ np.uint8(17 * k)).save(str(pictures / f'p{k}.png'))
    return dict(symbols=str(symbols), pictures=str(pictures))


def mode(resident):
    from vkit_amd import _native as N
    return N.resident(bool(resident))


def host_of(plane):
    from vkit_amd import _native as N
    if hasattr(plane, 'arr'):
        plane = plane.arr
    return N.host_array(plane)


def layout_of(**fields):
    from vkit_amd.pipeline.text_detection import PageLayout, PageLayoutStepOutput
    return PageLayoutStepOutput(page_layout=PageLayout(**fields))


def box_of(up, left, h, w):
    from vkit_amd.element import Box
    return Box(up=up, down=up + h - 1, left=left, right=left + w - 1)


# ---- every golden case through the public steps and engines ---------------------------------------------------------------------
def symbol_step(run, folders):
    from vkit_amd.pipeline import text_detection as T
    step = T.PageNonTextSymbolStep(T.PageNonTextSymbolStepConfig(symbol_image_folders=[folders['symbols']], **run['overrides']))
    step.selector.image_files[:] = [os.path.join(folders['symbols'], f + '.png') for f in run['files']]
    symbols = [T.LayoutNonTextSymbol(box=box_of(up, left, h, w), alpha=alpha) for up, left, h, w, alpha in run['layout']]
    return step, T.PageNonTextSymbolStepInput(page_layout_step_output=layout_of(height=160, width=200, layout_non_text_symbols=symbols))


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
def test_symbols_equal_golden_and_restatement(resident, folders):
    from vkit_amd import _native as N
    from vkit_amd.element import ScoreMap
    for run in INDEX['symbol_runs']:
        step, data = symbol_step(run, folders)
        rng = default_rng(run['seed'])
        with mode(resident):
            out = step.run(data, rng)
        assert rng.bit_generator.state == run['rng_state']
        assert len(out.images) == len(run['symbols']) and [b for b in out.boxes] == [s.box for s in data.page_layout_step_output.page_layout.layout_non_text_symbols]
        for image, alpha, row, (_, _, h, w, layout_alpha) in zip(out.images, out.alphas, run['symbols'], run['layout']):
            assert image.on_device == resident
            assert isinstance(alpha, ScoreMap if resident else np.ndarray)
            if resident:
                assert alpha.box is None and isinstance(alpha.arr, N.DevArray)
            src = TEXTURES[row['file']]
            want = R.symbol_rgba(src, (h, w), layout_alpha) if row['color'] is None else R.symbol_gray(src, (h, w), layout_alpha, row['color'])
            for got, golden, restated in ((image, GET(row['image']), want[0]), (alpha, GET(row['alpha']), want[1])):
                assert R.same_bits(host_of(got), golden), (run['name'], run['seed'])
                assert R.same_bits(host_of(got), restated), (run['name'], run['seed'])


def make_barcode_engine(kind, overrides):
    from vkit_amd.engine import barcode as B
    if kind == 'qr':
        return B.BarcodeQrEngine(B.BarcodeQrEngineInitConfig(**overrides), func_encode=R.qr_image)
    return B.BarcodeCode39Engine(B.BarcodeCode39EngineInitConfig(**overrides), func_encode=R.code39_image)


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
def test_barcode_engines_equal_golden_and_restatement(resident):
    from vkit_amd.engine.barcode import BarcodeEngineRunConfig
    for run in INDEX['barcode_runs']:
        engine = make_barcode_engine(run['kind'], run['overrides'])
        rng = default_rng(run['seed'])
        with mode(resident):
            score_map = engine.run(BarcodeEngineRunConfig(height=run['shape'][0], width=run['shape'][1]), rng)
        assert rng.bit_generator.state == run['rng_state']
        assert score_map.on_device == resident and score_map.is_prob and score_map.box is None
        assert R.same_bits(host_of(score_map), GET(run['score_map'])), run
        assert R.same_bits(host_of(score_map), R.score(GET(run['mask']), tuple(run['shape']), run['alpha'])[0]), run


def barcode_page_step():
    from vkit_amd.pipeline import text_detection as T
    page = R.BARCODE_PAGE
    step = T.PageBarcodeStep(T.PageBarcodeStepConfig(), func_encode_qr=R.qr_image, func_encode_code39=R.code39_image)
    return step, T.PageBarcodeStepInput(page_layout_step_output=layout_of(
        height=page['shape'][0], width=page['shape'][1], layout_barcode_qrs=[T.LayoutBarcodeQr(box=box_of(*b)) for b in page['qrs']],
        layout_barcode_code39s=[T.LayoutBarcodeCode39(box=box_of(*b)) for b in page['code39s']]))


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
def test_barcode_page_equals_golden(resident):
    page, stored = R.BARCODE_PAGE, INDEX['barcode_page']
    step, data = barcode_page_step()
    rng = default_rng(page['seed'])
    with mode(resident):
        out = step.run(data, rng)
    assert rng.bit_generator.state == stored['rng_state']
    assert (out.height, out.width) == tuple(page['shape'])
    for maps, entries, boxes in ((out.barcode_qr_score_maps, stored['qrs'], page['qrs']),
                                 (out.barcode_code39_score_maps, stored['code39s'], page['code39s'])):
        assert len(maps) == len(entries)
        for score_map, entry, b in zip(maps, entries, boxes):
            assert score_map.on_device == resident and score_map.box == box_of(*b)
            assert R.same_bits(host_of(score_map), GET(entry))


def frame_step(overrides):
    from vkit_amd.pipeline import text_detection as T
    return T.PageTextLineBoundingBoxStep(T.PageTextLineBoundingBoxStepConfig(**overrides))


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
def test_single_frames_equal_golden_and_restatement(resident):
    from vkit_amd.element import Box
    for row in INDEX['frames']:
        rng = default_rng(row['seed'])
        with mode(resident):
            score_map, color = frame_step(row['overrides']).sample_text_line_bounding_box(
                row['page'][0], row['page'][1], R.text_line_of(row['line_box'], row['ref_heights'], row['color'], Box), rng)
        assert rng.bit_generator.state == row['rng_state']
        assert list(color) == row['color'] and score_map.on_device == resident
        assert [score_map.box.up, score_map.box.down, score_map.box.left, score_map.box.right] == row['page_box']
        assert R.same_bits(host_of(score_map), GET(row['plane'])), row['name']
        assert R.same_bits(host_of(score_map), R.frame(row['box_shape'], row['thickness'], row['alpha'], row['trims'])), row['name']


def frame_page_input(seed):
    from vkit_amd.element import Box
    from vkit_amd.pipeline import text_detection as T
    lines = R.frame_run_lines(seed)
    collection = T.PageTextLineCollection(height=160, width=220, text_lines=[R.text_line_of(b, hs, c, Box) for b, hs, c, _ in lines],
                                          short_text_line_flags=[short for _, _, _, short in lines])
    return T.PageTextLineBoundingBoxStepInput(page_text_line_step_output=T.PageTextLineStepOutput(
        page_text_line_collection=collection,
        page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=160, width=220)))


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
def test_frame_pages_equal_golden(resident):
    for run in INDEX['frame_runs']:
        rng = default_rng(run['seed'])
        with mode(resident):
            out = frame_step(R.FRAME_RUN_CONFIG).run(frame_page_input(run['seed']), rng)
        assert rng.bit_generator.state == run['rng_state']
        assert [list(c) for c in out.colors] == [f['color'] for f in run['frames']]
        for score_map, row in zip(out.score_maps, run['frames']):
            assert score_map.on_device == resident
            assert R.same_bits(host_of(score_map), GET(row['plane']))


# ---- the launch and synchronisation budget --------------------------------------------------------------------------------------
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


def test_launch_and_sync_budget(monkeypatch, folders):
    """symbols: two launches for 1 and for 40; barcodes and frames: one; no synchronisation"""
    from vkit_amd import _native as N
    from vkit_amd.pipeline import text_detection as T
    ctx = N.default_ctx()
    files = [f for f in R.FILES if f != 'rgb_3ch']
    seen = []
    with N.resident(True):
        for n in (1, 40):
            layout = [(3 * k, 2 * k, 5 + k % 30, 7 + (k * 13) % 90, 0.5) for k in range(n)]
            run = dict(files=['rgba_9x7'] if n == 1 else files, layout=layout, overrides={})
            step, data = symbol_step(run, folders)
            plans = step.plan(data, default_rng(n))          # (the textures are decoded and cached here)
            step.render(plans)                               # warm the scratch slot
            out, launches, syncs = _count(monkeypatch, ctx, lambda: step.render(plans))
            seen.append((launches, syncs))
            assert len(out.images) == n
        assert seen[0] == seen[1] == ({'k_layer_symbols': 1, 'k_layer_planes': 1}, 0), seen

        step, data = barcode_page_step()
        plan = step.plan(data, default_rng(0))
        step.render(plan)
        _, launches, syncs = _count(monkeypatch, ctx, lambda: step.render(plan))
        assert (launches, syncs) == ({'k_layer_planes': 1}, 0)

        step = frame_step(R.FRAME_RUN_CONFIG)
        plans = step.plan(frame_page_input(0), default_rng(0))
        assert len(plans) > 1
        step.render(plans)
        _, launches, syncs = _count(monkeypatch, ctx, lambda: step.render(plans))
        assert (launches, syncs) == ({'k_layer_planes': 1}, 0)


# ---- the refusals of the C entry point ------------------------------------------------------------------------------------------
def valid_table():
    from vkit_amd.engine.page_layers import LayerBatch
    batch = LayerBatch()
    batch.add_symbol_rgba(TEXTURES['rgba_9x7'], (13, 11), 0.8)
    batch.add_symbol_gray(TEXTURES['gray_7x9'], (20, 33), 0.85, (1, 2, 3))
    batch.add_score(np.ones((5, 5), np.uint8), (8, 8), 0.7)
    batch.add_frame((20, 30), 2, 1.0, (1, 0, 2, 0))
    table, blob = batch.tables()
    return table, blob, batch.dst_bytes


def _set(field, value, row=0, item=None):
    def change(table):
        if item is None:
            table[field][row] = value
        else:
            table[field][row][item] = value
    return change


REFUSALS = {
    'unknown_kind': _set('kind', 9), 'negative_kind': _set('kind', -1),
    'src_side_zero': _set('src_h', 0), 'src_side_large': _set('src_w', 32768), 'out_side_zero': _set('out_w', 0),
    'out_side_large': _set('out_h', 32768), 'colour_high': _set('color', 256, 1, 2), 'colour_negative': _set('color', -1, 1, 0),
    'alpha_nan': _set('alpha', float('nan')), 'alpha_high': _set('alpha', 1.5, 2), 'alpha_negative': _set('alpha', -0.1, 3),
    'thickness_zero': _set('thickness', 0, 3), 'thickness_no_interior': _set('thickness', 10, 3),
    'trim_no_window': _set('trim', 19, 3, 1), 'trim_negative': _set('trim', -1, 3, 0), 'frame_output_not_window': _set('out_h', 18, 3),
    'blob_offset_out_of_range': _set('src_off', 1 << 20, 2), 'blob_offset_negative': _set('src_off', -2, 2),
    'no_device_source': _set('src_off', -1, 0),
    'image_outside_dst': _set('image_off', 1 << 30), 'plane_outside_dst': _set('alpha_off', 1 << 30, 2),
    'plane_negative': _set('alpha_off', -4, 2), 'plane_misaligned': _set('alpha_off', 2, 3),
}


@pytest.mark.parametrize('name', list(REFUSALS) + ['overlap', 'null_table', 'null_dst', 'null_blob', 'no_layers', 'too_many_layers',
                                                   'device_source_inside_dst'])
def test_refusals_launch_nothing(name):
    from ctypes import c_void_p
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    table, blob, dst_bytes = valid_table()
    dst = ctx.to_device(np.full(dst_bytes, 0xAB, np.uint8))
    args = dict(table=table.ctypes.data, n=len(table), blob=blob.ctypes.data, blob_bytes=blob.size, dst=dst.ptr)
    if name in REFUSALS:
        REFUSALS[name](table)
    elif name == 'overlap':
        table['alpha_off'][3] = table['alpha_off'][2]
    elif name == 'null_table':
        args['table'] = None
    elif name == 'null_dst':
        args['dst'] = None
    elif name == 'null_blob':
        args['blob'] = None
    elif name == 'no_layers':
        args['n'] = 0
    elif name == 'too_many_layers':
        args['n'] = 4097
    elif name == 'device_source_inside_dst':
        table['src_off'][0], table['src_dev'][0] = -1, dst.ptr + 256
    ctx.sync()
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        rc = N.lib().vkx_page_layers_dev(ctx.handle, args['table'], args['n'], args['blob'], args['blob_bytes'], c_void_p(args['dst']), dst_bytes)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    assert rc == N.ERR_INVALID
    assert 'vkx_page_layers_dev' in N.last_error()
    assert not timings, timings
    dst.invalidate_host()
    assert (dst.host() == 0xAB).all()


def test_the_valid_table_of_the_refusal_tests_runs():
    from vkit_amd import _native as N
    table, blob, dst_bytes = valid_table()
    dst = N.default_ctx().to_device(np.full(dst_bytes, 0xAB, np.uint8))
    N.page_layers(table, blob, dst)
    host = dst.host()
    got = host[table['alpha_off'][3]:table['alpha_off'][3] + 4 * 19 * 28].view(np.float32).reshape(19, 28)
    assert R.same_bits(got, R.frame((20, 30), 2, 1.0, (1, 0, 2, 0)))


# ---- a page with all four layer kinds, three ways -------------------------------------------------------------------------------
def test_a_page_assembled_three_ways(folders):
    from vkit_amd import _native as N
    from vkit_amd.element import Image, ScoreMap
    from vkit_amd.pipeline import text_detection as T
    page_h, page_w = R.BARCODE_PAGE['shape']
    symbol_run = [r for r in INDEX['symbol_runs'] if r['name'] == 'page0'][0]
    frame_run = INDEX['frame_runs'][0]
    image_step = T.PageImageStep(T.PageImageStepConfig(image_configs=[{'type': 'selector', 'config': {'image_folders': [folders['pictures']]}}]))
    image_step.image_engine_executor_aggregator.selector.engine_executors[0].engine.image_files.sort()
    image_boxes = [(10, 100, 40, 50), (120, 10, 30, 60), (60, 150, 25, 80)]
    layout = layout_of(height=page_h, width=page_w, layout_images=[T.LayoutImage(box=box_of(*b)) for b in image_boxes])

    def labels():
        return T.PageTextLineLabelStepOutput(
            page_char_polygon_collection=T.PageCharPolygonCollection(height=page_h, width=page_w),
            page_text_line_polygon_collection=T.PageTextLinePolygonCollection(height=page_h, width=page_w))

    def assemble(images, barcodes, frames, symbols):
        background = Image(mat=np.full((page_h, page_w, 3), 230, np.uint8))
        data = T.PageAssemblerStepInput(
            page_layout_step_output=layout, page_background_step_output=T.PageBackgroundStepOutput(background_image=background),
            page_image_step_output=images, page_barcode_step_output=barcodes,
            page_text_line_step_output=T.PageTextLineStepOutput(
                page_text_line_collection=T.PageTextLineCollection(height=page_h, width=page_w),
                page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=page_h, width=page_w)),
            page_non_text_symbol_step_output=symbols, page_text_line_bounding_box_step_output=frames,
            page_text_line_label_step_output=labels())
        return T.page_assembler_step_factory.create().run(data, default_rng(0)).page.image

    def from_steps(resident):
        with mode(resident):
            images = image_step.run(T.PageImageStepInput(page_layout_step_output=layout), default_rng(5))
            barcode_step, barcode_input = barcode_page_step()
            barcodes = barcode_step.run(barcode_input, default_rng(R.BARCODE_PAGE['seed']))
            frames = frame_step(R.FRAME_RUN_CONFIG).run(frame_page_input(frame_run['seed']), default_rng(frame_run['seed']))
            step, data = symbol_step(symbol_run, folders)
            symbols = step.run(data, default_rng(symbol_run['seed']))
            layers = ([p.image for p in images.page_image_collection.page_images] + list(barcodes.barcode_qr_score_maps)
                      + list(barcodes.barcode_code39_score_maps) + list(frames.score_maps) + list(symbols.images) + list(symbols.alphas))
            page = assemble(images, barcodes, frames, symbols)
            if resident:
                assert all(isinstance(layer.arr, N.DevArray) and layer.arr._host is None for layer in layers), 'a layer was downloaded'
            return np.array(page.mat), images

    host_page, host_images = from_steps(False)
    resident_page, _ = from_steps(True)

    # the golden planes handed over as plain containers
    page = R.BARCODE_PAGE
    barcodes = T.PageBarcodeStepOutput(
        height=page_h, width=page_w,
        barcode_qr_score_maps=[ScoreMap(mat=GET(e), box=box_of(*b)) for e, b in zip(INDEX['barcode_page']['qrs'], page['qrs'])],
        barcode_code39_score_maps=[ScoreMap(mat=GET(e), box=box_of(*b)) for e, b in zip(INDEX['barcode_page']['code39s'], page['code39s'])])
    from vkit_amd.element import Box
    frames = T.PageTextLineBoundingBoxStepOutput(
        score_maps=[ScoreMap(mat=GET(f['plane']), box=Box(*f['page_box'])) for f in frame_run['frames']],
        colors=[tuple(f['color']) for f in frame_run['frames']])
    symbols = T.PageNonTextSymbolStepOutput(
        images=[Image(mat=GET(row['image'])) for row in symbol_run['symbols']],
        boxes=[box_of(up, left, h, w) for up, left, h, w, _ in symbol_run['layout']],
        alphas=[np.array(GET(row['alpha'])) for row in symbol_run['symbols']])
    golden_page = np.array(assemble(host_images, barcodes, frames, symbols).mat)

    assert (golden_page != 230).any()
    assert (golden_page == host_page).all()
    assert (golden_page == resident_page).all()


# ---- a seeded random loop ------------------------------------------------------------------------------------------------------
def test_random_records_equal_the_restatement():
    from vkit_amd import _native as N
    from vkit_amd.engine.page_layers import LayerBatch
    rng = default_rng(20241106)
    ctx = N.default_ctx()
    for call in range(4):
        batch, want = LayerBatch(), []
        for k in range(50):
            kind = int(rng.integers(0, 4))
            alpha = float(rng.choice([0.0, 1.0, rng.uniform(0, 1)]))
            sh, sw = int(rng.integers(1, 30)), int(rng.integers(1, 40))
            oh, ow = (sh, sw) if rng.random() < 0.15 else (int(rng.integers(1, 40)), int(rng.integers(1, 150)))
            on_device = rng.random() < 0.5
            if kind == 0:
                src = rng.integers(0, 256, size=(sh, sw, 4)).astype(np.uint8)
                if rng.random() < 0.1:
                    src[:, :, 3] = 0
                batch.add_symbol_rgba(ctx.to_device(src) if on_device else src, (oh, ow), alpha)
                want.append(R.symbol_rgba(src, (oh, ow), alpha))
            elif kind == 1:
                src = R.blocky(rng, (sh, sw), 3, 0, 2) * np.uint8(rng.integers(1, 256))
                color = tuple(int(v) for v in rng.integers(0, 256, 3))
                batch.add_symbol_gray(ctx.to_device(src) if on_device else src, (oh, ow), alpha, color)
                want.append(R.symbol_gray(src, (oh, ow), alpha, color))
            elif kind == 2:
                mask = R.blocky(rng, (sh, sw), 2, 0, 2)
                batch.add_score(mask, (oh, ow), alpha)
                want.append((None, R.score(mask, (oh, ow), alpha)[0]))
            else:
                thick = int(rng.integers(1, 5))
                bh, bw = 2 * thick + 2 + int(rng.integers(0, 30)), 2 * thick + 2 + int(rng.integers(0, 120))
                trims = (int(rng.integers(0, bh // 2)), int(rng.integers(0, bh // 2)), int(rng.integers(0, bw // 2)), int(rng.integers(0, bw // 2)))
                batch.add_frame((bh, bw), thick, alpha, trims)
                want.append((None, R.frame((bh, bw), thick, alpha, trims)))
        for k, ((image, plane), (want_image, want_plane)) in enumerate(zip(batch.render(resident=bool(call % 2)), want)):
            assert (image is None) == (want_image is None)
            if image is not None:
                assert R.same_bits(host_of(image), want_image), (call, k)
            assert R.same_bits(host_of(plane), want_plane), (call, k, batch.records[k])
