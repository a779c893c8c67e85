"""The image engines and PageBackgroundStep on the GPU (vkit_amd/engine/image/, csrc/image_combine.hip): the engines against the
reference's own runs (tests/golden/image_engine.npz) on host arrays and device-resident, the raw entry point against the
restatement (tests/image_engine_restate.py) on tile tables the planner would not produce, the launch / synchronisation /
download budget, the resident hand-over to PageAssemblerStep, ABI refusals, the texture cache under a small budget and a
seeded soak.  Everything is integer arithmetic: exact equality throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_engine_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

TEXTURES, METAS, CASES = R.load()
BY_FILE = {'image/' + R.texture_name(k): t for k, t in enumerate(TEXTURES)}


@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    """{texture subset: folder with image/ + metas.json}; the files keep their fixture names."""
    root = tmp_path_factory.mktemp('textures')
    made = {}

    def folder(indices):
        key = tuple(indices)
        if key not in made:
            path = str(root / ('set_' + '_'.join(map(str, key))))
            R.write_folder(path, TEXTURES, METAS)
            # the subset: metas.json lists only its files
            import json
            rows = [dict(image_file=R.texture_name(k), grayscale_mean=float(METAS[k][0]), grayscale_std=float(METAS[k][1])) for k in key]
            with open(os.path.join(path, 'metas.json'), 'w') as fout:
                json.dump(rows, fout)
            made[key] = path
        return made[key]

    return folder


def _files(folder, indices):
    return [os.path.join(folder, 'image', R.texture_name(k)) for k in indices]


def _check(image, case, resident):
    from vkit_amd import _native as N
    from vkit_amd.element import ImageMode
    assert isinstance(image.arr, N.DevArray) == resident
    mat = image.mat
    assert mat.dtype == np.uint8 and mat.shape == case['want'].shape and mat.tobytes() == case['want'].tobytes()
    assert image.mode == ImageMode(case['mode'])


def _combiner_groups():
    groups = {}
    for c in CASES:
        if c['kind'] == 'combiner':
            groups.setdefault((c['case'], c['seed']), []).append(c)
    return [sorted(g, key=lambda c: c['run']) for g in groups.values()]


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('group', _combiner_groups(), ids=lambda g: R.case_id(g[0]))
def test_combiner_equals_the_reference(group, resident, folders):
    from vkit_amd import _native as N
    from vkit_amd.engine.image import ImageCombinerEngine, ImageEngineRunConfig
    first = group[0]
    engine = ImageCombinerEngine(R.combiner_config(first, folders(first['metas'])))
    rng = default_rng(first['seed'])
    for case in group:
        with N.resident(resident):
            image = engine.run(ImageEngineRunConfig(height=case['shape'][0], width=case['shape'][1]), rng)
        assert rng.bit_generator.state == case['rng_state']
        _check(image, case, resident)


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', [c for c in CASES if c['kind'] == 'selector'], ids=R.case_id)
def test_selector_equals_the_reference(case, resident, folders):
    from vkit_amd import _native as N
    from vkit_amd.element import ImageMode
    from vkit_amd.engine.image import ImageEngineRunConfig, ImageSelectorEngine, ImageSelectorEngineInitConfig
    folder = folders(range(len(TEXTURES)))
    overrides = dict(case['overrides'])
    if overrides.get('target_image_mode'):
        overrides['target_image_mode'] = ImageMode(overrides['target_image_mode'])
    engine = ImageSelectorEngine(ImageSelectorEngineInitConfig(image_folders=[folder], **overrides),
                                 image_files=_files(folder, case['files']))
    rng = default_rng(case['seed'])
    with N.resident(resident):
        image = engine.run(ImageEngineRunConfig(**case['run_config']), rng)
    assert rng.bit_generator.state == case['rng_state']
    _check(image, case, resident)


def test_selector_globs_its_folders(folders):
    from vkit_amd.engine.image import ImageSelectorEngine, ImageSelectorEngineInitConfig
    folder = folders(range(len(TEXTURES)))
    engine = ImageSelectorEngine(ImageSelectorEngineInitConfig(image_folders=[folder]))
    assert sorted(os.path.basename(str(f)) for f in engine.image_files) == [R.texture_name(k) for k in range(len(TEXTURES))]


def _background_step(case, folders):
    from vkit_amd.pipeline.text_detection import PageBackgroundStepConfig, page_background_step_factory
    image_configs = []
    for kind, weight, overrides, files in case['engines']:
        config = dict(overrides)
        if kind == 'combiner':
            config['image_meta_folder'] = folders(files)
        else:
            config['image_folders'] = [folders(range(len(TEXTURES)))]
        image_configs.append(dict(type=kind, weight=weight, config=config))
    step = page_background_step_factory.create(PageBackgroundStepConfig(image_configs=image_configs, **case['overrides']))
    for executor, (kind, _, _, files) in zip(step.image_engine_executor_aggregator.selector.engine_executors, case['engines']):
        if kind == 'selector':
            executor.engine.image_files = _files(folders(range(len(TEXTURES))), files)
    return step


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', [c for c in CASES if c['kind'] == 'background'], ids=R.case_id)
def test_background_step_equals_the_reference(case, resident, folders):
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import PageBackgroundStepInput, PageShapeStepOutput
    step = _background_step(case, folders)
    rng = default_rng(case['seed'])
    with N.resident(resident):
        out = step.run(PageBackgroundStepInput(PageShapeStepOutput(height=case['shape'][0], width=case['shape'][1])), rng)
    assert rng.bit_generator.state == case['rng_state']
    _check(out.background_image, case, resident)


def test_background_step_reads_a_json_path(tmp_path, folders):
    import json
    from vkit_amd.pipeline.text_detection import page_background_step_factory
    path = tmp_path / 'image_configs.json'
    path.write_text(json.dumps([dict(type='combiner', config=dict(image_meta_folder=folders(range(len(TEXTURES)))))]))
    step = page_background_step_factory.create(dict(image_configs=str(path)))
    assert len(step.image_engine_executor_aggregator.selector.engine_executors) == 1


# ---- the raw entry point ------------------------------------------------------------------------------------------------
def _random_table(rng, shape, sources, n_tiles, one_pixel=False):
    h, w = shape
    tiles = []
    for _ in range(n_tiles):
        s = int(rng.integers(0, len(sources)))
        sh, sw = sources[s].shape[:2]
        th = 1 if one_pixel else int(rng.integers(1, min(sh, h) + 1))
        tw = 1 if one_pixel else int(rng.integers(1, min(sw, w) + 1))
        up, left = int(rng.integers(0, h - th + 1)), int(rng.integers(0, w - tw + 1))
        tiles.append((up, up + th - 1, left, left + tw - 1, s))
    return tiles


RAW_SHAPES = [(50, 70), (16, 64), (17, 65), (100, 129), (1, 9), (9, 1), (3, 2), (130, 40), (33, 200)]


@pytest.mark.parametrize('ksize', [3, 5, 7])
@pytest.mark.parametrize('shape', RAW_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_raw_entry_equals_the_restatement(shape, ksize):
    """overlapping tiles, uncovered pixels, one-pixel tiles, tiles on the last row and column, bands at all four borders"""
    from vkit_amd import _native as N
    rng = default_rng(shape[0] * 1000 + shape[1] * 10 + ksize)
    sources = [rng.integers(0, 256, (int(rng.integers(1, 60)), int(rng.integers(1, 90)), 3), dtype=np.uint8) for _ in range(5)]
    h, w = shape
    tables = [
        _random_table(rng, shape, sources, 6),
        _random_table(rng, shape, sources, 40),
        _random_table(rng, shape, sources, 30, one_pixel=True),
        [],
        # the four corners and the last row / column
        [(0, 0, 0, 0, 0), (h - 1, h - 1, w - 1, w - 1, 1), (0, 0, w - 1, w - 1, 2), (h - 1, h - 1, 0, 0, 3),
         (h - 1, h - 1, 0, min(w, sources[4].shape[1]) - 1, 4), (0, min(h, sources[4].shape[0]) - 1, w - 1, w - 1, 4)],
    ]
    half = ksize // 2 + 1
    for k, tiles in enumerate(tables):
        for resident in (False, True):
            with N.resident(resident):
                got = N.image_combine(tiles, sources, shape, ksize, half / 3)
            assert isinstance(got, N.DevArray) == resident
            want = R.combine(tiles, sources, shape, ksize)
            assert np.array_equal(N.host_array(got), want), (k, resident)
    # a band other than the reference's
    tiles = tables[1]
    for half_width, sigma in ((0, 1.0), (1, 0.7), (6, 2.0)):
        got = N.image_combine(tiles, sources, shape, ksize, sigma, half=half_width)
        assert np.array_equal(got, R.combine(tiles, sources, shape, ksize, half=half_width, sigma=sigma)), half_width


def test_raw_entry_at_the_block_borders():
    """A 40 x 150 page (3 x 3 blocks of 64 x 16), ksize 5 and half 3, so a tile reaches 3 pixels beyond its edges: tiles whose right
    edge is 60 (the reach ends on the block's last column), 61 (one column into the next block) and 64 (inside it), and whose lower
    edge is 12, 13 and 16 likewise; each alone, and the nine in one table."""
    from vkit_amd import _native as N
    rng = default_rng(405)
    shape, ksize, half = (40, 150), 5, 3
    sources = [rng.integers(0, 256, (20, 70, 3), dtype=np.uint8), rng.integers(0, 256, (18, 66, 3), dtype=np.uint8)]
    tiles = [(1, down, 2, right, (down + right) % 2) for down in (15 - half, 16 - half, 16) for right in (63 - half, 64 - half, 64)]
    for k, table in enumerate([[t] for t in tiles] + [tiles]):
        got = N.image_combine(table, sources, shape, ksize, 1.0, half=half)
        assert np.array_equal(got, R.combine(table, sources, shape, ksize, half=half, sigma=1.0)), k


# ---- budget ----------------------------------------------------------------------------------------------------------------
def _big_folder(tmp_path, n=6, side=256, seed=0):
    rng = default_rng(seed)
    textures = [np.repeat(np.repeat(rng.integers(0, 256, (side // 8, side // 8, 3), dtype=np.uint8), 8, axis=0), 8, axis=1)
                for _ in range(n)]
    metas = [(100.0 + k, 10.0) for k in range(n)]
    return R.write_folder(str(tmp_path / 'big'), textures, metas), textures, metas


class _Counters:
    def __init__(self, monkeypatch):
        from vkit_amd import _native as N
        self.syncs, self.downloads, self.uploads = [], [], []
        real = {name: getattr(N.Context, name) for name in ('sync', 'download', 'download_async', 'copy_out', 'upload')}
        monkeypatch.setattr(N.Context, 'sync', lambda s: self.syncs.append(1) or real['sync'](s))
        for name in ('download', 'download_async', 'copy_out'):
            monkeypatch.setattr(N.Context, name, (lambda n: lambda s, *a, **k: self.downloads.append(n) or real[n](s, *a, **k))(name))
        monkeypatch.setattr(N.Context, 'upload', lambda s, *a, **k: self.uploads.append(1) or real['upload'](s, *a, **k))


def test_warm_run_is_one_launch(tmp_path, monkeypatch):
    """A combiner run on warm textures inside resident(True): one k_image_combine, no other kernel, no Context.sync, no copy to
    the host; the first run adds one upload per first-seen file and at most one warp per first-seen rotated file.  As in the
    heatmap's budget test, synchronisation is watched at the Python wrapper: a stream synchronisation inside the library (its
    table slot growing, the page-locked ring wrapping) is not seen here; the slot starts at 256 KB so that warm runs do not grow it."""
    from vkit_amd import _native as N
    from vkit_amd.engine.image import ImageCombinerEngine, ImageCombinerEngineInitConfig, ImageEngineRunConfig
    folder, textures, _ = _big_folder(tmp_path)
    engine = ImageCombinerEngine(ImageCombinerEngineInitConfig(image_meta_folder=folder, prob_use_only_the_anchor_image=0.0, sigma=30.0))
    ctx = N.default_ctx()
    run_config = ImageEngineRunConfig(height=1024, width=1024)
    ctx.sync()
    counters = _Counters(monkeypatch)
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        with N.resident(True):
            engine.run(run_config, default_rng(0))
        first = ctx.timings()
        first_uploads, first_downloads = len(counters.uploads), len(counters.downloads)
        # every (file, flag) of later runs is cached once both flags of every file have been seen: run until warm
        for seed in range(1, 12):
            with N.resident(True):
                engine.run(run_config, default_rng(seed))
        cache = engine.texture_cache(ctx)
        if len(cache) < 2 * len(textures):
            pytest.fail(f'the warm-up left {len(cache)} of {2 * len(textures)} textures cached')
        ctx.reset_timings()
        del counters.syncs[:], counters.downloads[:], counters.uploads[:]
        with N.resident(True):
            image = engine.run(run_config, default_rng(99))
        warm_syncs, warm_downloads, warm_uploads = list(counters.syncs), list(counters.downloads), list(counters.uploads)
        warm = ctx.timings()
    finally:
        ctx.set_timing(0)
    assert isinstance(image.arr, N.DevArray)
    assert {name: cnt for name, (_ms, cnt) in warm.items() if cnt} == {'k_image_combine': 1}, warm
    assert warm_syncs == [] and warm_downloads == [] and warm_uploads == []
    launches = {name: cnt for name, (_ms, cnt) in first.items() if cnt}
    assert launches.pop('k_image_combine') == 1
    assert sum(launches.values()) <= len(textures), first         # warps of first-seen rotated files, nothing else
    assert 1 <= first_uploads <= len(textures) and first_downloads == 0
    # and the warm page is the restatement's
    want_engine = R.Combiner(engine.init_config, engine.image_metas, {m.image_file: t for m, t in zip(
        sorted(engine.image_metas, key=lambda m: m.image_file), textures)})
    _, want = want_engine.run(1024, 1024, default_rng(99))
    assert np.array_equal(image.mat, want)


def test_resident_background_reaches_the_assembler_without_a_download(tmp_path, monkeypatch):
    from vkit_amd import _native as N
    from vkit_amd.element import Image
    from vkit_amd.pipeline import text_detection as T
    from vkit_amd.pipeline.text_detection.synthetic_page import synthetic_page_input
    folder, _, _ = _big_folder(tmp_path, side=128)
    step = T.page_background_step_factory.create(dict(
        image_configs=[dict(type='combiner', config=dict(image_meta_folder=folder))], weight_image=1.0, weight_random_grayscale=0.0))
    size = 256
    shape_input = T.PageBackgroundStepInput(T.PageShapeStepOutput(height=size, width=size))
    page_input = synthetic_page_input(seed=3, size=size, n_lines=24)
    assembler = T.page_assembler_step_factory.create()
    # the same background as a host array: today's path
    with N.resident(False):
        host_background = step.run(shape_input, default_rng(4)).background_image
    assert isinstance(host_background.arr, np.ndarray)
    page_input.page_background_step_output = T.PageBackgroundStepOutput(Image(mat=np.array(host_background.mat)))
    want = np.array(assembler.run(page_input, default_rng(0)).page.image.mat)
    # device-resident: not downloaded on the way
    counters = _Counters(monkeypatch)
    hosts = []
    real_host = N.DevArray.host
    monkeypatch.setattr(N.DevArray, 'host', lambda self: hosts.append(self.shape) or real_host(self))
    with N.resident(True):
        background = step.run(shape_input, default_rng(4)).background_image
        assert isinstance(background.arr, N.DevArray)
        page_input.page_background_step_output = T.PageBackgroundStepOutput(background)
        page = assembler.run(page_input, default_rng(0)).page
    # (the seal impression's rotated planes are device arrays in resident mode and are read back as layer planes, as before:
    # small, and not the background)
    assert (size, size, 3) not in hosts and background.arr._host is None
    assert isinstance(page.image.arr, N.DevArray) and page.image.arr is not background.arr
    assert np.array_equal(page.image.mat, want)
    # the background itself is untouched by the composite
    assert np.array_equal(background.mat, host_background.mat)
    # a grey page is born on the device too
    grey = T.page_background_step_factory.create(dict(
        image_configs=[dict(type='combiner', config=dict(image_meta_folder=folder))], weight_image=0.0, weight_random_grayscale=1.0))
    a, b = default_rng(8), default_rng(8)
    with N.resident(True):
        dev = grey.run(shape_input, a).background_image
    host = grey.run(shape_input, b).background_image
    assert isinstance(dev.arr, N.DevArray) and isinstance(host.arr, np.ndarray)
    assert np.array_equal(dev.mat, host.mat) and a.bit_generator.state == b.bit_generator.state


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_canaries():
    from vkit_amd import _native as N
    L = N.lib()
    ctx = N.default_ctx()
    h, w = 40, 50
    canary = np.full((h, w, 3), 0xAB, np.uint8)
    dst = ctx.to_device(canary)
    big = ctx.to_device(np.full((h + 10, w + 10, 3), 0x11, np.uint8))
    src = ctx.to_device(default_rng(0).integers(0, 256, (20, 30, 3), dtype=np.uint8))

    def tiles(*rows):
        arr = (N.VkxCombineTile * max(1, len(rows)))()
        for rec, row in zip(arr, rows):
            rec.up, rec.down, rec.left, rec.right, rec.source = row
        return arr, len(rows)

    def sources(*arrays):
        arr = (N.VkxCombineSource * max(1, len(arrays)))()
        for rec, a in zip(arr, arrays):
            rec.image, rec.height, rec.width = (a.ptr, a.shape[0], a.shape[1]) if a is not None else (None, 4, 4)
        return arr, len(arrays)

    good_tiles, good_sources = tiles((0, 19, 0, 29, 0)), sources(src)

    def call(t=good_tiles, s=good_sources, ksize=5, half=3, sigma=1.0, out=dst.ptr, hh=h, ww=w, handle=ctx.handle):
        return L.vkx_image_combine_u8c3_dev(handle, t[0], t[1], s[0], s[1], ksize, half, sigma, ctypes.c_void_p(out), hh, ww)

    inside = ctypes.c_void_p(big.ptr + 3 * (w + 10) + 3)      # a destination inside a source's bytes
    refused = dict(
        null_ctx=lambda: call(handle=None),
        null_dst=lambda: call(out=None),
        null_tiles=lambda: L.vkx_image_combine_u8c3_dev(ctx.handle, None, 1, good_sources[0], 1, 5, 3, 1.0, ctypes.c_void_p(dst.ptr), h, w),
        null_sources=lambda: L.vkx_image_combine_u8c3_dev(ctx.handle, good_tiles[0], 1, None, 1, 5, 3, 1.0, ctypes.c_void_p(dst.ptr), h, w),
        null_source_image=lambda: call(s=sources(None)),
        negative_h=lambda: call(hh=-1),
        negative_w=lambda: call(ww=-1),
        huge_h=lambda: call(hh=(1 << 19) + 1, t=tiles()),
        huge_w=lambda: call(ww=(1 << 19) + 1, t=tiles()),
        huge_area=lambda: call(hh=1 << 15, ww=1 << 14, t=tiles()),
        even_ksize=lambda: call(ksize=4),
        zero_ksize=lambda: call(ksize=0),
        negative_ksize=lambda: call(ksize=-3),
        ksize_above_cap=lambda: call(ksize=17),
        negative_half=lambda: call(half=-1),
        half_above_cap=lambda: call(half=65),
        zero_sigma=lambda: call(sigma=0.0),
        nan_sigma=lambda: call(sigma=float('nan')),
        tile_below_page=lambda: call(t=tiles((30, 40, 0, 9, 0))),
        tile_right_of_page=lambda: call(t=tiles((0, 9, 45, 50, 0))),
        tile_negative=lambda: call(t=tiles((-1, 9, 0, 9, 0))),
        tile_inverted=lambda: call(t=tiles((9, 8, 0, 9, 0))),
        tile_taller_than_source=lambda: call(t=tiles((0, 20, 0, 9, 0))),
        tile_wider_than_source=lambda: call(t=tiles((0, 9, 0, 30, 0))),
        source_index_high=lambda: call(t=tiles((0, 9, 0, 9, 1))),
        source_index_negative=lambda: call(t=tiles((0, 9, 0, 9, -1))),
        overlap=lambda: L.vkx_image_combine_u8c3_dev(ctx.handle, good_tiles[0], 1, sources(big)[0], 1, 5, 3, 1.0, inside, h, w),
    )
    for name, fn in refused.items():
        assert fn() == N.ERR_INVALID, name
        ctx.sync()
        assert np.array_equal(ctx.download(dst.ptr, np.empty_like(canary)), canary), name
        assert (ctx.download(big.ptr, np.empty(big.shape, np.uint8)) == 0x11).all(), name
    # an empty page is accepted and writes nothing
    assert call(hh=0, t=tiles()) == 0
    ctx.sync()
    assert np.array_equal(ctx.download(dst.ptr, np.empty_like(canary)), canary)
    # one good call on the same context
    assert call() == 0
    got = ctx.download(dst.ptr, np.empty_like(canary))
    assert np.array_equal(got, R.combine([(0, 19, 0, 29, 0)], [src.host()], (h, w), 5, half=3, sigma=1.0))


def test_oversized_bin_table_is_refused_early():
    """Large overlapping tiles: more than 2^26 (block, tile) pairs are refused while they are counted, nothing written."""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    side = 2048                                   # 32 x 128 blocks
    src = N.dev_full((side, side, 3), 0x22, ctx=ctx)
    dst = N.dev_full((side, side, 3), 0xAB, ctx=ctx)
    n = (1 << 26) // (32 * 128) + 1
    tiles = (N.VkxCombineTile * n)()
    view = N.struct_view(tiles)
    view['down'][:] = side - 1
    view['right'][:] = side - 1
    source = (N.VkxCombineSource * 1)()
    source[0].image, source[0].height, source[0].width = src.ptr, side, side
    rc = N.lib().vkx_image_combine_u8c3_dev(ctx.handle, tiles, n, source, 1, 5, 3, 1.0, ctypes.c_void_p(dst.ptr), side, side)
    assert rc == N.ERR_INVALID
    assert (dst.host() == 0xAB).all()
    # one tile fewer than the cap's worth is a table like any other
    rc = N.lib().vkx_image_combine_u8c3_dev(ctx.handle, tiles, 8, source, 1, 5, 3, 1.0, ctypes.c_void_p(dst.ptr), side, side)
    assert rc == 0
    dst.invalidate_host()
    got = dst.host()
    assert (got == 0x22).all()


def test_selector_never_hands_out_its_cache_entry(folders):
    """The whole file (disable_resizing, or a window as large as the file) is returned as a copy in both modes."""
    from vkit_amd import _native as N
    from vkit_amd.engine.image import ImageEngineRunConfig, ImageSelectorEngine, ImageSelectorEngineInitConfig
    folder = folders(range(len(TEXTURES)))
    engine = ImageSelectorEngine(ImageSelectorEngineInitConfig(image_folders=[folder]), image_files=_files(folder, [11]))
    h, w = TEXTURES[11].shape[:2]
    ctx = N.default_ctx()
    for run_config in (dict(height=0, width=0, disable_resizing=True), dict(height=h, width=w)):
        for resident in (True, False):
            with N.resident(resident):
                image = engine.run(ImageEngineRunConfig(**run_config), default_rng(0))
            cached = engine.texture(ctx, _files(folder, [11])[0])
            assert np.array_equal(image.mat, TEXTURES[11])
            if resident:
                assert image.arr is not cached and image.arr.ptr != cached.ptr
            else:
                assert not np.shares_memory(image.arr, cached.host())
                with image.writable_context:
                    image.mat[:] = 0
            assert np.array_equal(cached.host(), TEXTURES[11])


# ---- the texture cache -------------------------------------------------------------------------------------------------------
def test_small_cache_budget_gives_golden_output(folders):
    """A byte budget below the texture set: textures are dropped and decoded again, no draw changes."""
    from vkit_amd import _native as N
    from vkit_amd.engine.image import ImageCombinerEngine, ImageEngineRunConfig
    budget = 6000          # the set holds 12 textures of up to 17 280 bytes
    assert sum(t.nbytes for t in TEXTURES) > 10 * budget
    for group in _combiner_groups():
        first = group[0]
        if first['case'] not in ('several_metas', 'cache_on', 'cache_off', 'rotate_half'):
            continue
        engine = ImageCombinerEngine(R.combiner_config(first, folders(first['metas'])), cache_bytes=budget)
        rng = default_rng(first['seed'])
        for case in group:
            image = engine.run(ImageEngineRunConfig(height=case['shape'][0], width=case['shape'][1]), rng)
            assert rng.bit_generator.state == case['rng_state']
            assert image.mat.tobytes() == case['want'].tobytes()
            cache = engine.texture_cache(N.default_ctx())
            assert cache.bytes <= budget
        if first['overrides'].get('enable_cache'):
            # the recorded flags outlive the dropped textures
            flagged = set(engine.image_file_to_rotate_flag)
            assert flagged and {key[0] for key in cache.items} <= flagged


# ---- soak --------------------------------------------------------------------------------------------------------------------
def test_seeded_soak_against_the_restatement(folders):
    """400 seeded runs of random engine configurations and page shapes up to 1024^2, device-resident, against the restatement
    (about 10 s; the count is fixed, the time is what the machine makes of it)."""
    from vkit_amd import _native as N
    from vkit_amd.engine.image import ImageCombinerEngine, ImageCombinerEngineInitConfig, ImageEngineRunConfig
    rng = default_rng(2024)
    runs = 0
    while runs < 400:
        n = int(rng.integers(1, len(TEXTURES) + 1))
        indices = sorted(int(k) for k in rng.choice(len(TEXTURES), size=n, replace=False))
        ksize = int(rng.choice([3, 5, 7]))
        config_cls = type('SoakInitConfig', (ImageCombinerEngineInitConfig,), dict(gaussian_blur_kernel_size=ksize))
        overrides = dict(prob_use_only_the_anchor_image=float(rng.choice([0.0, 0.7, 1.0])), prob_rotate_image=float(rng.random()),
                         enable_cache=bool(rng.integers(0, 2)), sigma=float(rng.choice([1.0, 3.0, 30.0])),
                         init_segment_width_min_ratio=float(rng.choice([0.1, 0.25, 0.5])))
        folder = folders(indices)
        engine = ImageCombinerEngine(config_cls(image_meta_folder=folder, **overrides), cache_bytes=int(rng.choice([4000, 1 << 30])))
        want_engine = R.Combiner(config_cls(image_meta_folder=folder, **overrides),
                                 R.metas_of(indices, METAS, prefix=os.path.join(folder, 'image') + os.sep),
                                 {os.path.join(folder, 'image', R.texture_name(k)): TEXTURES[k] for k in indices})
        seed = int(rng.integers(0, 1 << 30))
        a, b = default_rng(seed), default_rng(seed)
        for _ in range(int(rng.integers(1, 4))):
            big = rng.random() < 0.1
            height = int(rng.integers(1, 1025 if big else 200))
            width = int(rng.integers(2, 1025 if big else 200))
            if min(TEXTURES[k].shape[0] for k in indices) < 12 and height * width > 300 * 300:
                height, width = min(height, 300), min(width, 300)       # tens of thousands of tiny tiles: the host plan, not the kernel
            with N.resident(True):
                image = engine.run(ImageEngineRunConfig(height=height, width=width), a)
            tiles, want = want_engine.run(height, width, b)
            assert a.bit_generator.state == b.bit_generator.state
            assert np.array_equal(image.mat, want), (runs, indices, overrides, ksize, seed, height, width, len(tiles))
            runs += 1
    assert runs >= 400
