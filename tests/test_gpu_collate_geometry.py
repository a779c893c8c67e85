"""GPU: the batch collate (csrc/collate.hip) past its first workgroup and at its numeric edges, against tests/collate_restate.py,
bit for bit and between canaries.  An image workgroup is 256 lanes x 2 groups x 4 pixels = 2048 pixels, a lane's second group
starts at pixel 1024; a plane workgroup is 8192 bytes, a lane's second 16-byte group starts at byte 4096, the bytes past a record's
last 16 are written singly, and the workgroup that owns a record is found by bisection.  One process, one context (and a cold one
for the growth of the record table)."""
import ctypes
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collate_restate as R  # noqa: E402
from collate_gpu_cases import CANARY, _carve, _mods, _samples  # noqa: E402

pytestmark = pytest.mark.gpu

# (h, w): what the pixel count reaches
BOUNDARY_SHAPES = [(1, 1), (1, 2), (1, 3),      # 1 .. 3 pixels: no whole group, the tail lanes only
                   (32, 32),                    # 1024: the first group of all 256 lanes, the second of none
                   (13, 79),                    # 1027: the same and a 3-pixel tail
                   (4, 257),                    # 1028: one lane has a second group
                   (32, 64),                    # 2048: exactly one workgroup
                   (7, 293),                    # 2051: one workgroup and a tail that lies past the last group
                   (27, 76),                    # 2052: a second workgroup of one group
                   (41, 100),                   # 4100: three workgroups, the last nearly empty
                   (3, 1367)]                   # 4101: three workgroups and a 1-pixel tail
PLANE_SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 4111, 4112, 8191, 8192, 8193, 8208, 12288, 16389, 24576 + 4097]
ALIGNMENTS = {'wide': (0, 0), 'src+1': (1, 0), 'dst+4': (0, 4), 'both+8': (8, 8)}       # (source, destination) mod 16


def _check_batch(torch, TB, samples, host, **kw):
    """One collate into fresh tensors and one into ``out=`` tensors between canaries, every output against the restatement."""
    restated = {k: kw[k] for k in ('mean', 'std') if k in kw}
    want = {'page_image': R.collate_images(host['page_image'], kw['image_dtype'], channels_first=kw['channels_first'], **restated)}
    want.update({key: R.collate_planes(planes) for key, planes in host.items() if key != 'page_image'})
    got = TB.collate_cropped_pages(samples, **kw)
    assert set(got) == set(want) | {'target_core_box', 'downsampled_target_core_box'}
    wanted = {key: (tuple(got[key].shape), got[key].dtype) for key in want}
    buffer, out, used = _carve(torch, got['page_image'].device, wanted)
    again = TB.collate_cropped_pages(samples, out=out, **kw)
    for key, w in want.items():
        assert got[key].is_contiguous() and tuple(got[key].shape) == tuple(w.shape), key
        assert R.same_bits(got[key], w), key
        assert again[key] is out[key] and R.same_bits(again[key], w), key
    assert (buffer.cpu().numpy()[~used] == CANARY).all(), 'a byte outside the outputs was written'
    return want


# ---- 1. the image kernel at its group and workgroup boundaries ---------------------------------------------------------------
@pytest.mark.parametrize('channels_first', [True, False], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('shape', BOUNDARY_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_collate_images_at_group_and_workgroup_boundaries(shape, dtype, channels_first):
    """n = 3 with the sources at byte offsets 0 .. 3 (sample i one further, mod 4), n = 1 at offset 1 only (the other three offsets
    of n = 1 are dropped: the first sample of the n = 3 runs has them); labels of 6 and 24 bytes; fresh outputs, then ``out=`` tensors
    between canaries."""
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    rng = default_rng(1000 * shape[0] + shape[1])
    for n, first_offset in [(3, 0), (3, 1), (3, 2), (3, 3), (1, 1)]:
        samples, host = _samples(N, ctx, rng, n, shape, (2, 3), first_offset)
        _check_batch(torch, TB, samples, host, image_dtype=dtype, channels_first=channels_first)


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------
def _raw_collate(N, ctx, image_ptrs=(), planes=(), norm=None):
    """One vkx_collate_dev call: ``image_ptrs`` the sources, ``planes`` (src, dst, bytes) records, ``norm`` the fields of the
    vkx_collate_norm (``mean`` and ``scale`` the float32 constants) or None for NULL.  -> the return code."""
    image_ptrs = np.asarray(image_ptrs, np.uint64)
    image_table = (N.VkxCollateImage * max(1, len(image_ptrs)))()
    if len(image_ptrs):
        np.frombuffer(image_table, np.uint64)[:] = image_ptrs
    plane_table = (N.VkxCollatePlane * max(1, len(planes)))()
    if len(planes):
        np.frombuffer(plane_table, np.uint64).reshape(-1, 3)[:] = np.asarray(planes, np.uint64)
    nrm = None
    if norm is not None:
        nrm = N.VkxCollateNorm()
        norm = dict(norm)
        nrm.mean[:], nrm.scale[:] = [float(v) for v in norm.pop('mean')], [float(v) for v in norm.pop('scale')]
        for key, value in norm.items():
            setattr(nrm, key, value)
    return N.lib().vkx_collate_dev(ctx.handle, image_table if len(image_ptrs) else None, len(image_ptrs),
                                   plane_table if len(planes) else None, len(planes), ctypes.byref(nrm) if nrm is not None else None)


class _Device:
    """Plain device blocks of one context for a raw call: uploaded on the way in, downloaded whole, freed at the end."""

    def __init__(self, ctx):
        self.ctx, self.blocks = ctx, []

    def put(self, array):
        ptr = self.ctx.malloc(array.nbytes)
        self.blocks.append(ptr)
        self.ctx.upload(ptr, array)
        assert ptr % 16 == 0
        return ptr

    def get(self, ptr, nbytes):
        self.ctx.sync()
        return self.ctx.download(ptr, np.empty(nbytes, np.uint8))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        for ptr in self.blocks:
            self.ctx.free(ptr)


def _run_planes(N, ctx, rng, records):
    """``records`` (bytes, source mod 16, destination mod 16) as ONE call: the sources at those residues in one random buffer, the
    destinations in one canary-filled buffer with 32 .. 47 canary bytes between them; every byte of the destination buffer -- the
    copies and the canaries between and around them -- is checked."""
    src_at, dst_at, s, d = [], [], 16, 48
    for nbytes, s_mod, d_mod in records:
        src_at.append(s + s_mod)
        dst_at.append(d + d_mod)
        s = (s + s_mod + nbytes + 15) // 16 * 16 + 16
        d = (d + d_mod + nbytes + 15) // 16 * 16 + 32
    source = rng.integers(0, 256, (s,), dtype=np.uint8)
    source[source == CANARY] = 0x5A                                         # a copied byte never looks like an untouched one
    want = np.full((d + 16,), CANARY, np.uint8)
    for (nbytes, _, _), sa, da in zip(records, src_at, dst_at):
        want[da:da + nbytes] = source[sa:sa + nbytes]
    with _Device(ctx) as dev:
        src, dst = dev.put(source), dev.put(np.full_like(want, CANARY))
        table = [(src + sa, dst + da, nbytes) for (nbytes, _, _), sa, da in zip(records, src_at, dst_at)]
        assert all(p[0] % 16 == r[1] and p[1] % 16 == r[2] for p, r in zip(table, records))
        assert _raw_collate(N, ctx, planes=table) == 0, N.last_error()
        got = dev.get(dst, want.size)
        assert (dev.get(src, source.size) == source).all()
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f'{wrong.size} bytes differ, the first at {wrong[0]} of {want.size}: records at {dst_at[:8]} ...'
    return sum(r[0] for r in records)


# ---- 2. grid limits ---------------------------------------------------------------------------------------------------------
def test_collate_65535_images_in_one_call():
    """gridDim.y at its limit: 65535 (1, 2) images six bytes apart in one buffer, float16 NHWC, no planes."""
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    n = 65535
    raw = default_rng(21).integers(0, 256, (6 * n,), dtype=np.uint8)
    want = R.collate_images(raw.reshape(n, 1, 2, 3), 'float16', channels_first=False)
    m, s = R.constants()
    with _Device(ctx) as dev:
        src = dev.put(raw)
        batch = dev.put(np.full((want.nbytes + 96,), CANARY, np.uint8))
        norm = dict(dst=batch + 48, height=1, width=2, dtype=TB.COLLATE_F16, channels_first=0, mean=m, scale=s)
        assert _raw_collate(N, ctx, image_ptrs=src + 6 * np.arange(n, dtype=np.uint64), norm=norm) == 0, N.last_error()
        got = dev.get(batch, want.nbytes + 96)
    assert (got[:48] == CANARY).all() and (got[48 + want.nbytes:] == CANARY).all()
    assert R.same_bits(got[48:48 + want.nbytes].view(np.float16).reshape(want.shape), want)


def test_collate_images_only_and_planes_only():
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    rng = default_rng(22)
    h, w, n = 5, 7, 2
    m, s = R.constants()
    images = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    want = R.collate_images(images, 'float32')
    with _Device(ctx) as dev:
        src = dev.put(images)
        batch = dev.put(np.full((want.nbytes + 96,), CANARY, np.uint8))
        norm = dict(dst=batch + 48, height=h, width=w, dtype=TB.COLLATE_F32, channels_first=1, mean=m, scale=s)
        assert _raw_collate(N, ctx, image_ptrs=[src, src + h * w * 3], norm=norm) == 0, N.last_error()          # n_planes = 0
        got = dev.get(batch, want.nbytes + 96)
    assert (got[:48] == CANARY).all() and (got[48 + want.nbytes:] == CANARY).all()
    assert R.same_bits(got[48:48 + want.nbytes].view(np.float32).reshape(want.shape), want)
    assert _run_planes(N, ctx, rng, [(100, 0, 0), (33, 3, 5)]) == 133                                            # n_images = 0, norm = NULL


# ---- 3. the plane kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alignment', list(ALIGNMENTS))
def test_collate_plane_records_alone(alignment):
    """Each size alone in a call: the whole-workgroup sizes, the sizes around a lane's second group (4096) and around the workgroup
    (8192), records of up to four workgroups; 16 bytes a lane where both ends are aligned, single bytes otherwise."""
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    rng = default_rng(30 + sum(ALIGNMENTS[alignment]))
    for nbytes in PLANE_SIZES:
        _run_planes(N, ctx, rng, [(nbytes,) + ALIGNMENTS[alignment]])


def test_collate_plane_records_mixed_in_one_table():
    """Every size in every alignment in ONE table, in a seeded shuffled order: one-workgroup records between records of several, so
    the bisection has to find every record from every one of its workgroups."""
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    rng = default_rng(34)
    records = [(nbytes,) + mods for nbytes in PLANE_SIZES for mods in ALIGNMENTS.values()]
    records = [records[i] for i in rng.permutation(len(records))]
    assert len(records) == 64 and sum(-(-r[0] // 8192) for r in records) == 4 * 24
    assert _run_planes(N, ctx, rng, records) == 4 * sum(PLANE_SIZES)


def _small_call(N, TB, ctx, rng):
    """The small valid call of the refusal test (one (6, 8) float32 image, one 64-byte plane), on random bytes."""
    h, w = 6, 8
    image, plane = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (64,), dtype=np.uint8)
    m, s = np.array([1.0, 2.0, 3.0], np.float32), np.array([0.5, 0.25, 0.125], np.float32)
    want = np.ascontiguousarray(((image.astype(np.float32) - m) * s).transpose(2, 0, 1))
    with _Device(ctx) as dev:
        src, plane_src = dev.put(image), dev.put(plane)
        batch, plane_dst = dev.put(np.full((want.nbytes + 64,), CANARY, np.uint8)), dev.put(np.full((128,), CANARY, np.uint8))
        norm = dict(dst=batch, height=h, width=w, dtype=TB.COLLATE_F32, channels_first=1, mean=m, scale=s)
        assert _raw_collate(N, ctx, image_ptrs=[src], planes=[(plane_src, plane_dst, 64)], norm=norm) == 0, N.last_error()
        got, got_plane = dev.get(batch, want.nbytes + 64), dev.get(plane_dst, 128)
    assert R.same_bits(got[:want.nbytes].view(np.float32).reshape(want.shape), want) and (got[want.nbytes:] == CANARY).all()
    assert (got_plane[:64] == plane).all() and (got_plane[64:] == CANARY).all()


def _small_records(rng, n):
    """n records of 1 .. 40 bytes, half of them 16-byte aligned at both ends, the others at random residues."""
    return [(int(b), 0 if a else int(sm), 0 if a else int(dm)) for b, a, sm, dm in
            zip(rng.integers(1, 41, n), rng.random(n) < 0.5, rng.integers(0, 16, n), rng.integers(0, 16, n))]


def test_collate_record_table_grows_past_its_first_allocation():
    """On a context of its own, so that the size of the device table is known at every step.  The first, small call reserves the
    site's minimum of 64 KB plus the slack every scratch block gets (bytes + bytes / 8 + 256): 73 984 bytes.  3000 records (72 000
    bytes of table behind the 256-byte image part) still fit that block; 4000 records (96 000 bytes) do not: the call synchronises,
    frees the block the calls before used and allocates a larger one.  The small call follows each of them.  All exact."""
    torch, N, TB = _mods()
    record, first_cap = ctypes.sizeof(N.VkxCollatePlane), (64 << 10) + (64 << 10) // 8 + 256
    assert record == 24 and first_cap == 73984 and 256 + 3000 * record <= first_cap < 4000 * record
    ctx = N.Context(N.default_ctx().device)
    try:
        rng = default_rng(35)
        _small_call(N, TB, ctx, rng)
        for n in (3000, 4000):
            records = _small_records(rng, n)
            assert _run_planes(N, ctx, rng, records) == sum(r[0] for r in records)
            _small_call(N, TB, ctx, rng)
    finally:
        ctx.close()


@pytest.mark.parametrize('channels_first', [True, False], ids=['nchw', 'nhwc'])
def test_collate_labels_of_several_workgroups(channels_first):
    """Through the public function, n = 3: (3, 2731) labels are uint8 planes of 8193 bytes (two workgroups, the second with one
    byte) and float32 planes of 32772, their shrunk forms 1365 and 5460 bytes; the planes of samples 1 and 2 land off the 16-byte
    grid in their batch, so the same call takes the byte path for them and the 16-byte path for sample 0."""
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    samples, host = _samples(N, ctx, default_rng(36), 3, (5, 5), (3, 2731), 1)
    want = _check_batch(torch, TB, samples, host, image_dtype='float16', channels_first=channels_first)
    assert want['page_char_mask'][0].nbytes == 8193 and want['page_char_height_score_map'][0].nbytes == 32772
    assert want['downsampled_page_char_mask'][0].nbytes == 1365 and want['downsampled_page_text_line_height_score_map'][0].nbytes == 5460


# ---- 4. arithmetic edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_first', [True, False], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('name', list(R.EDGE_CONSTANTS))
def test_collate_arithmetic_edges(name, dtype, channels_first):
    """Every byte value in every channel under constants that reach subnormal, infinite and signed-zero outputs (counted on the
    restatement first, so the case cannot stop reaching them unnoticed); never a NaN."""
    torch, N, TB = _mods()
    from vkit_amd.element import Image
    ctx = N.default_ctx()
    mean, std = R.EDGE_CONSTANTS[name]
    found = R.classes(R.collate_images([R.edge_image()], dtype, mean, std, channels_first=channels_first))
    assert all(found[c] > 0 for c in R.EDGE_REACHES[name].get(dtype, ())) and found['nan'] == 0 and found['size'] == 768, found
    samples, host = _samples(N, ctx, default_rng(40), 2, (16, 16), (2, 3), 0)
    samples[1].page_image = Image(mat=ctx.to_device(R.edge_image()))
    host['page_image'][1] = R.edge_image()
    want = _check_batch(torch, TB, samples, host, image_dtype=dtype, channels_first=channels_first, mean=mean, std=std)
    assert R.classes(want['page_image'])['nan'] == 0


# ---- 6. the collate between torch's streams ---------------------------------------------------------------------------------
def test_collate_orders_itself_between_the_writes_and_reads_of_a_side_stream(monkeypatch):
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    syncs = []
    real_sync = N.Context.sync
    rng = default_rng(60)
    samples, host = _samples(N, ctx, rng, 2, (41, 100), (2, 3), 0)
    base = np.minimum(host['page_image'][0], 200).astype(np.uint8)                       # room for + 5
    arr = ctx.to_device(base)
    samples[0].page_image = type(samples[0].page_image)(mat=arr)
    first = TB.collate_cropped_pages(samples, image_dtype='float32')         # the shapes and dtypes of the batch
    wanted = {key: (tuple(t.shape), t.dtype) for key, t in first.items() if t.is_cuda}
    ctx.sync()
    torch.cuda.synchronize()
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = TB.as_tensor(arr)
        for _ in range(20):                       # torch writes the source through the view on ITS stream ...
            t.add_(1)
            t.sub_(1)
        t.add_(5)
        buffer, out, used = _carve(torch, t.device, wanted)                  # ... and fills the outputs there just before
        for tensor in out.values():
            tensor.fill_(1)
        assert arr._viewed == {int(side.cuda_stream)}
        batch = TB.collate_cropped_pages(samples, image_dtype='float32', out=out)
        consumed = batch['page_image'].to(torch.int32)                       # ... and reads the batch at once
        labels = {key: batch[key].to(torch.int32) for key in wanted if key != 'page_image'}
    assert not syncs
    assert arr._viewed == {int(side.cuda_stream)}
    side.synchronize()
    want = R.collate_images([base + 5, host['page_image'][1]], 'float32')
    assert np.array_equal(consumed.cpu().numpy(), want.astype(np.int32))
    assert R.same_bits(batch['page_image'], want)
    for key, planes in host.items():
        if key != 'page_image':
            assert R.same_bits(batch[key], R.collate_planes(planes)), key
            assert np.array_equal(labels[key].cpu().numpy(), R.collate_planes(planes).astype(np.int32)), key
    assert (buffer.cpu().numpy()[~used] == CANARY).all()
