"""The JPEG encoder on the device (csrc/jpeg_encode.hip, vkx_jpeg_encode_u8_dev): byte for byte the files Pillow's libjpeg-turbo
writes (tests/golden/jpeg_encode.npz), alone and batched, through _native.jpeg_encode, Image.to_file / to_jpeg_bytes and
encode_jpeg_images; the capacity contract with a canary; the refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from jpeg_encode_cases import golden_cases  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1
CANARY = 0xA5


@pytest.fixture(scope='module')
def N():
    from vkit_amd import _native
    return _native


def _records(N, arrays):
    records = (N.VkxJpegImage * max(len(arrays), 1))()
    for rec, arr in zip(records, arrays):
        rec.src, rec.h, rec.w, rec.cn = arr.ptr, arr.shape[0], arr.shape[1], 1 if arr.ndim == 2 else arr.shape[2]
    return records


def _raw(N, ctx, records, n, quality, bgr, out, capacity, offsets):
    """the C entry point on caller-owned device buffers; returns its code, synchronised"""
    rc = N.lib().vkx_jpeg_encode_u8_dev(ctx.handle, records, n, quality, bgr, ctypes.c_void_p(out.ptr if out is not None else None),
                                        capacity, ctypes.c_void_p(offsets.ptr if offsets is not None else None))
    ctx.sync()
    return rc


def _filled(ctx, nbytes, dtype=np.uint8):
    host = np.full(nbytes, CANARY, np.uint8).view(dtype)
    return ctx.to_device(host), host


def _host(ctx, dev):
    dev.invalidate_host()
    return np.array(dev.host())


def test_every_golden_case_alone(N, golden_dir):
    for name, mat, q, want in golden_cases(golden_dir):
        got = N.jpeg_encode([mat], quality=q)
        assert len(got) == 1 and isinstance(got[0], bytes)
        assert got[0] == want, (name, q, len(got[0]), len(want))


def test_batches_of_one_quality_equal_the_single_calls(N, golden_dir):
    ctx = N.default_ctx()
    for quality in (1, 10, 50, 75, 95, 100):
        cases = [c for c in golden_cases(golden_dir) if c[2] == quality]
        assert len(cases) >= 20 and {c[1].ndim for c in cases} == {2, 3}
        got = N.jpeg_encode([c[1] for c in cases], quality=quality)
        assert got == [c[3] for c in cases], quality
        # the offsets are the running sum of the sizes
        devs = [ctx.to_device(np.ascontiguousarray(c[1])) for c in cases]
        total = sum(len(c[3]) for c in cases)
        out, offsets = N.jpeg_encode_raw(_records(N, devs), len(devs), quality, False, total, ctx)
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(c[3]) for c in cases])]).tolist()
        assert _host(ctx, out).tobytes() == b''.join(c[3] for c in cases)


def test_scans_cross_their_rounds(N, golden_dir):
    """The three scans (an image's blocks, its chunks, the images of a call) walk their range a round at a time with a carry:
    128 entries a round for ranges up to 2048, 8192 beyond.  256 x 256 RGB has 1536 blocks (12 small rounds) and 156 chunks
    (2); a call of 293 images takes 3 small rounds of the offsets scan, one of 8492 images 2 large ones."""
    ctx = N.default_ctx()
    small, small_max, large = N.JPEG_SCAN_SMALL_ROUND, N.JPEG_SCAN_SMALL_MAX, N.JPEG_SCAN_LARGE_ROUND
    cases = golden_cases(golden_dir)
    big = [c for c in cases if c[0].startswith('256x256x3')]
    nblk = 6 * 16 * 16
    nchunks = -(-nblk * 208 // 2048)
    assert big and 8 * small < nblk <= small_max and small < nchunks <= small_max
    for name, mat, q, want in big:
        assert N.jpeg_encode([mat], quality=q) == [want], (name, q)
    tiny = [c for c in cases if c[2] == 75 and c[1].shape[0] * c[1].shape[1] <= 81]
    assert len(tiny) >= 20 and {c[1].ndim for c in tiny} == {2, 3}
    devs = [ctx.to_device(np.ascontiguousarray(c[1])) for c in tiny]
    page = next(c for c in big if c[2] == 75)
    page_dev = ctx.to_device(np.ascontiguousarray(page[1]))
    for count in (2 * small + 37, large + 300):
        assert (small < count <= small_max) or count > max(large, small_max)
        # the tiny images in turn (a stride coprime to their number, so that a round's sizes differ from the next one's), one page
        # in the middle: the files after it start past a block scan and a chunk scan of several rounds
        picks = [(7 * i) % len(tiny) for i in range(count)]
        images = [devs[k] for k in picks]
        want = [tiny[k][3] for k in picks]
        images[count // 2], want[count // 2] = page_dev, page[3]
        got = N.jpeg_encode(images, quality=75)
        assert len(got) == count
        wrong = [i for i in range(count) if got[i] != want[i]]
        assert not wrong, (count, wrong[:5])


def test_large_scan_shape_crosses_a_round_of_blocks(N):
    """The 8192-a-round shape of the block scan is reached only by an image of more than 2048 blocks and crosses a round only past
    8192, which no 256 x 256 image has: a thin grey strip of 33 x 32768 makes 5 x 4096 = 20 480 blocks (3 large rounds) and 2080
    chunks (the large shape of the chunk scan, one round).  The expected file is the restatement's, which the CPU tests pin."""
    import jpeg_encode_restate as E
    h, w = 33, 32768
    nblk = -(-h // 8) * (w // 8)
    assert nblk > 2 * N.JPEG_SCAN_LARGE_ROUND and -(-nblk * 208 // 2048) > N.JPEG_SCAN_SMALL_MAX
    yy, xx = np.indices((h, w))
    mat = ((xx // 5 + yy * 3) % 256).astype(np.uint8)
    want, census = E.encode(mat, 50)
    assert census['stuffed'] > 100
    # alone, and behind and before small images in one call
    assert N.jpeg_encode([mat], quality=50) == [want]
    small = mat[:9, :9].copy()
    assert N.jpeg_encode([small, mat, small], quality=50) == [E.encode_bytes(small, 50), want, E.encode_bytes(small, 50)]


def test_bgr_on_the_flipped_input_and_device_arrays(N, golden_dir):
    ctx = N.default_ctx()
    cases = [c for c in golden_cases(golden_dir) if c[2] in (50, 100)]
    colour = [c for c in cases if c[1].ndim == 3]
    assert any('asymmetric' in c[0] for c in colour)
    flipped = [np.ascontiguousarray(c[1][..., ::-1]) for c in colour]
    for quality in (50, 100):
        pick = [i for i, c in enumerate(colour) if c[2] == quality]
        assert N.jpeg_encode([flipped[i] for i in pick], quality=quality, bgr=True) == [colour[i][3] for i in pick]
        # grey images take no notice of bgr
        grey = [c for c in cases if c[1].ndim == 2 and c[2] == quality]
        assert N.jpeg_encode([c[1] for c in grey], quality=quality, bgr=True) == [c[3] for c in grey]
        # device arrays, host arrays and a mix of the two
        some = [c for c in cases if c[2] == quality][:12]
        mixed = [ctx.to_device(np.ascontiguousarray(c[1])) if i % 2 else c[1] for i, c in enumerate(some)]
        assert N.jpeg_encode(mixed, quality=quality) == [c[3] for c in some]
        assert N.jpeg_encode([ctx.to_device(np.ascontiguousarray(c[1])) for c in some], quality=quality) == [c[3] for c in some]


def test_small_capacity_keeps_to_it_reports_the_sizes_and_the_wrapper_retries(N, golden_dir):
    ctx = N.default_ctx()
    cases = [c for c in golden_cases(golden_dir) if c[2] == 95][:16]
    want = b''.join(c[3] for c in cases)
    sizes = [len(c[3]) for c in cases]
    devs = [ctx.to_device(np.ascontiguousarray(c[1])) for c in cases]
    records = _records(N, devs)
    # capacities inside a header, inside a scan, at a file boundary, one short of the total, zero
    for capacity in (100, sizes[0] + 700, sizes[0] + sizes[1], len(want) - 1, 0):
        out, _ = _filled(ctx, len(want) + 64)
        offsets, _ = _filled(ctx, 8 * (len(cases) + 1), np.int64)
        assert _raw(N, ctx, records, len(cases), 95, 0, out, capacity, offsets) == 0
        got = _host(ctx, out)
        assert got[:capacity].tobytes() == want[:capacity], capacity
        assert (got[capacity:] == CANARY).all(), capacity                       # nothing at or past the capacity
        assert _host(ctx, offsets).tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    # the wrapper: a first call at the small capacity, one more at the reported size
    calls = []
    raw = N.jpeg_encode_raw

    def counting(records, n, quality, bgr, capacity, ctx):
        calls.append(int(capacity))
        return raw(records, n, quality, bgr, capacity, ctx)

    N.jpeg_encode_raw = counting
    try:
        assert N.jpeg_encode([c[1] for c in cases], quality=95, capacity=100) == [c[3] for c in cases]
        assert calls == [100, len(want)]
        del calls[:]
        assert N.jpeg_encode([c[1] for c in cases], quality=95) == [c[3] for c in cases]
        assert calls == [sum(c[1].nbytes for c in cases) + 1024 * len(cases)]           # the default is enough: one call
    finally:
        N.jpeg_encode_raw = raw


def test_refusals_write_nothing(N):
    ctx = N.default_ctx()
    img = ctx.to_device(np.random.default_rng(0).integers(0, 256, (24, 40, 3), dtype=np.uint8))
    out, out_before = _filled(ctx, 8192)
    offsets, offsets_before = _filled(ctx, 8 * 4, np.int64)

    def record(**fields):
        recs = _records(N, [img])
        for key, value in fields.items():
            setattr(recs[0], key, value)
        return recs

    good = dict(records=record(), n=1, quality=75, bgr=0, out=out, capacity=8192, offsets=offsets)
    refused = [dict(records=None), dict(out=None), dict(offsets=None), dict(records=record(src=None)),
               dict(n=0), dict(n=-1), dict(n=65536),
               dict(records=record(h=0)), dict(records=record(h=32769)), dict(records=record(w=0)), dict(records=record(w=32769)),
               dict(records=record(cn=0)), dict(records=record(cn=2)), dict(records=record(cn=4)),
               dict(quality=-1), dict(quality=101), dict(bgr=2), dict(bgr=-1), dict(capacity=-1)]
    for change in refused:
        args = dict(good, **change)
        assert _raw(N, ctx, args['records'], args['n'], args['quality'], args['bgr'], args['out'], args['capacity'],
                    args['offsets']) == INVALID, change
        assert 'vkx_jpeg_encode_u8_dev' in N.last_error()
    # out or offsets overlapping the source: the source is its own destination here
    big = ctx.to_device(np.full(24 * 40 * 3 + 64, 7, np.uint8))
    inside = N.DevView(big, 0, (24, 40, 3))
    for change in (dict(out=N.DevView(big, 24 * 40 * 3 - 1, (65,)), capacity=65), dict(offsets=N.DevView(big, 16, (2,), np.int64))):
        args = dict(good, records=_records(N, [inside]), **change)
        assert _raw(N, ctx, args['records'], 1, 75, 0, args['out'], args['capacity'], args['offsets']) == INVALID, change
    assert (_host(ctx, big) == 7).all()
    assert (_host(ctx, out) == out_before).all() and (_host(ctx, offsets) == offsets_before).all()
    # and the good call goes through
    assert _raw(N, ctx, **good) == 0
    assert _host(ctx, offsets)[0] == 0 and 623 < _host(ctx, offsets)[1] < 8192
    with pytest.raises(ValueError):
        N.jpeg_encode([np.zeros((4, 4, 4), np.uint8)])
    with pytest.raises(ValueError):
        N.jpeg_encode([np.zeros((4, 4), np.uint8)], quality=101)
    with pytest.raises(TypeError):
        N.jpeg_encode([np.zeros((4, 4), np.float32)])
    assert N.jpeg_encode([]) == []


def test_image_to_file(N, golden_dir, tmp_path):
    from vkit_amd.element import Image, ImageMode
    ctx = N.default_ctx()
    cases = [c for c in golden_cases(golden_dir) if c[2] == 75]
    assert {c[1].ndim for c in cases} == {2, 3} and len(cases) >= 20
    for i, (name, mat, _q, want) in enumerate(cases):
        # device-resident and host images in turn; a grey image stays grey only with the RGB conversion disabled
        image = Image(mat=ctx.to_device(np.ascontiguousarray(mat)) if i % 2 else np.array(mat))
        for path in (tmp_path / 'a.jpg', tmp_path / 'b.JPEG'):
            image.to_file(path, disable_to_rgb_image=mat.ndim == 2)
            assert path.read_bytes() == want, (name, path.name)
        assert image.to_jpeg_bytes() == want
    # a grey image is written as RGB by default, as the reference does: the file of the grey-to-RGB mat
    name, mat, _q, _want = next(c for c in cases if c[1].ndim == 2 and c[1].size > 64)
    Image(mat=np.array(mat)).to_file(tmp_path / 'grey.jpe')
    assert (tmp_path / 'grey.jpe').read_bytes() == N.jpeg_encode([np.stack([mat] * 3, axis=-1)])[0]
    # an RGBA image under a JPEG extension raises, and writes nothing
    rgba = Image(mat=np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(OSError):
        rgba.to_file(tmp_path / 'rgba.jfif', disable_to_rgb_image=True)
    assert not (tmp_path / 'rgba.jfif').exists()
    # an HSV image with the conversion disabled: the mat as it stands
    name, mat, _q, want = next(c for c in cases if c[1].ndim == 3 and c[1].size > 64)
    hsv = Image(mat=np.array(mat), mode=ImageMode.HSV)
    hsv.to_file(tmp_path / 'hsv.jpg', disable_to_rgb_image=True)
    assert (tmp_path / 'hsv.jpg').read_bytes() == want
    hsv.to_file(tmp_path / 'rgb.jpg')
    assert (tmp_path / 'rgb.jpg').read_bytes() == hsv.to_rgb_image().to_jpeg_bytes() != want
    # quality reaches the encoder
    name, mat, q, want = next(c for c in golden_cases(golden_dir) if c[2] == 10 and c[1].ndim == 3)
    assert Image(mat=np.array(mat)).to_jpeg_bytes(quality=10) == want


def test_image_to_file_png_reads_back(N, tmp_path):
    pytest.importorskip('PIL')
    from vkit_amd.element import Image
    mat = np.random.default_rng(5).integers(0, 256, (33, 47, 3), dtype=np.uint8)
    Image(mat=N.default_ctx().to_device(mat)).to_file(tmp_path / 'c.png')
    back = Image.from_file(tmp_path / 'c.png')
    assert (back.mat == mat).all()
    assert (np.asarray(Image(mat=mat).to_pil_image()) == mat).all()


def test_encode_jpeg_images_over_mixed_shapes(N, golden_dir):
    from vkit_amd.element import Image, encode_jpeg_images
    ctx = N.default_ctx()
    cases = [c for c in golden_cases(golden_dir) if c[2] == 50]
    assert len({c[1].shape for c in cases}) >= 10
    images = [Image(mat=ctx.to_device(np.ascontiguousarray(c[1])) if i % 3 else np.array(c[1])) for i, c in enumerate(cases)]
    assert encode_jpeg_images(images, quality=50) == [c[3] for c in cases]
    assert encode_jpeg_images([]) == []
    with pytest.raises(OSError):
        encode_jpeg_images([Image(mat=np.zeros((8, 8, 4), np.uint8))])
