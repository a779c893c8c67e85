"""vkit_amd.torch_bridge without a GPU: the collate's arithmetic against a second formulation, the host plan, every refusal that
is decided before a device is touched, the array interface of a DevArray, and the stream bookkeeping of views and borrowed
tensors (on a context whose ordering calls are recorded instead of made)."""
import ctypes
import gc
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import collate_restate as R
from vkit_amd import _native as N
from vkit_amd import torch_bridge as TB
from vkit_amd.element import Box, Image, Mask, ScoreMap
from vkit_amd.pipeline.text_detection.page_cropping import CroppedPage, DownsampledLabel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DTYPES = {'uint8': torch.uint8, 'float32': torch.float32, 'float16': torch.float16, 'bfloat16': torch.bfloat16}


# ---- the restatement against torch CPU ops ---------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_first', [True, False])
@pytest.mark.parametrize('dtype', R.DTYPES)
def test_restatement_agrees_with_torch_cpu_ops(dtype, channels_first):
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (16, 17, 3), dtype=np.uint8) for _ in range(3)]
    images[0].reshape(-1)[:768] = np.repeat(np.arange(256), 3)   # every byte value in every channel
    got = R.collate_images(images, dtype, channels_first=channels_first)

    x = torch.stack([torch.from_numpy(i) for i in images])
    if dtype != 'uint8':
        m = torch.tensor([255.0 * v for v in R.MEAN], dtype=torch.float64).to(torch.float32)
        s = (1.0 / (255.0 * torch.tensor(R.STD, dtype=torch.float64))).to(torch.float32)
        x = x.to(torch.float32).sub(m).mul(s)
    if channels_first:
        x = x.permute(0, 3, 1, 2)
    want = x.contiguous().to(TORCH_DTYPES[dtype])
    assert tuple(want.shape) == ((3, 3, 16, 17) if channels_first else (3, 16, 17, 3))
    assert R.same_bits(got, want)


@pytest.mark.parametrize('name', list(R.EDGE_CONSTANTS))
def test_restatement_equals_a_float64_evaluation_at_the_edge_constants(name):
    """Every byte value in every channel.  float64(x) - float64(m) is exact (an integer below 256 against a float32), and the test
    asserts that it fits float32, so the restatement's float32 subtraction did not round; its product with float64(s) is exact too
    (24 + 24 bits of 53); ONE rounding to float32 -- to a subnormal, to zero or to infinity where the set goes there -- is the batch."""
    mean, std = R.EDGE_CONSTANTS[name]
    image = R.edge_image()
    m, s = R.constants(mean, std)
    assert m.dtype == s.dtype == np.float32 and np.isfinite(m).all() and np.isfinite(s).all() and (s != 0).all()
    diff = image.astype(np.float64) - m.astype(np.float64)
    assert (diff.astype(np.float32).astype(np.float64) == diff).all()
    product = diff * s.astype(np.float64)
    assert np.isfinite(product).all() and ((product != 0) | (diff == 0)).all()                    # float64 has the room
    mantissa, _ = np.frexp(product)
    assert (mantissa * 2.0 ** 48 == np.round(mantissa * 2.0 ** 48)).all()                           # 48 bits: nothing was rounded off
    with np.errstate(over='ignore', under='ignore'):
        want = product.astype(np.float32)
    got = R.collate_images([image], 'float32', mean, std, channels_first=False)
    assert got.dtype == np.float32 and R.same_bits(got, want[None])
    assert R.same_bits(R.collate_images([image], 'float32', mean, std), np.ascontiguousarray(want.transpose(2, 0, 1))[None])
    for dtype, reached in R.EDGE_REACHES[name].items():
        found = R.classes(R.collate_images([image], dtype, mean, std))
        assert all(found[c] > 0 for c in reached) and found['nan'] == 0, (dtype, found)


@pytest.mark.parametrize('channels_first', [True, False])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('name', list(R.EDGE_CONSTANTS))
def test_restatement_agrees_with_torch_cpu_ops_at_the_edge_constants(name, dtype, channels_first):
    mean, std = R.EDGE_CONSTANTS[name]
    rng = np.random.default_rng(6)
    images = [R.edge_image()] + [rng.integers(0, 256, (16, 16, 3), dtype=np.uint8) for _ in range(2)]
    got = R.collate_images(images, dtype, mean, std, channels_first=channels_first)
    m = (255.0 * torch.tensor(mean, dtype=torch.float64)).to(torch.float32)
    s = (1.0 / (255.0 * torch.tensor(std, dtype=torch.float64))).to(torch.float32)
    assert R.same_bits(m, R.constants(mean, std)[0]) and R.same_bits(s, R.constants(mean, std)[1])
    x = torch.stack([torch.from_numpy(i) for i in images]).to(torch.float32).sub(m).mul(s)
    if channels_first:
        x = x.permute(0, 3, 1, 2)
    want = x.contiguous().to(TORCH_DTYPES[dtype])
    assert R.same_bits(got, want)
    found = R.classes(got)
    assert all(found[c] > 0 for c in R.EDGE_REACHES[name].get(dtype, ())) and found['nan'] == 0, found


def test_bridge_constants_are_the_restatement_s():
    m, s = TB.norm_constants(R.MEAN, R.STD)
    rm, rs = R.constants()
    assert m.dtype == s.dtype == np.float32 and R.same_bits(m, rm) and R.same_bits(s, rs)
    # rounded once from float64: not the float32 product / quotient
    assert float(m[0]) == float(np.float32(255.0 * 0.485)) and float(s[2]) == float(np.float32(1.0 / (255.0 * 0.225)))
    for mean, std in R.EDGE_CONSTANTS.values():                            # subnormal scales and scales near the top of float32 included
        m, s = TB.norm_constants(mean, std)
        assert R.same_bits(m, R.constants(mean, std)[0]) and R.same_bits(s, R.constants(mean, std)[1])


def test_norm_constants_refuse_what_float32_cannot_hold():
    for kw, message in ((dict(std=(1e-41, 1, 1)), r'std\[0\] = 1e-41'), (dict(std=(1, 1e-320, 1)), r'std\[1\] = 1e-320'),
                        (dict(std=(1, 1, -1e-41)), r'std\[2\] = -1e-41'), (dict(mean=(2e36, 0, 0)), r'mean\[0\] = 2e\+36'),
                        (dict(mean=(0, 0, -2e36)), r'mean\[2\] = -2e\+36')):
        with pytest.raises(ValueError, match=message + '.*not finite'):
            TB.norm_constants(**{'mean': (0, 0, 0), 'std': (1, 1, 1), **kw})
    m, s = TB.norm_constants((1.3e36, 0, 0), (1e308, 1.2e-41, 1e36))        # the largest of their kind that float32 still holds
    assert np.isfinite(m).all() and np.isfinite(s).all() and s[0] == 0 and s[1] > 3e38 and 0 < s[2] < 1e-38


# ---- the host plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1, 2, 3])
@pytest.mark.parametrize('width', [1, 3, 4, 5, 8])
def test_plan_groups_tail_and_plane_paths(width, offset):
    height, n, base, dst = 3, 2, 0x7F0000100000, 0x7F0000900000
    pixels = height * width
    sources = [base + offset + 4096 * i for i in range(n)]
    planes = [(base + 65536 + offset, dst + 1024, pixels),                       # a uint8 mask out of a view
              (base + 131072, dst + 2048 + 16 * offset, 4 * pixels),             # a float32 map, destination aligned for offset 0 only ...
              (base + 196608, dst + 4096, 20000)]                                # ... and a plane of more than one workgroup
    plan = TB.collate_plan(sources, (height, width), 'float32', dst, planes)
    assert plan['images'] == sources                                              # any byte alignment goes down as it is
    assert (plan['groups'], plan['tail']) == (pixels // 4, pixels % 4) and plan['groups'] * 4 + plan['tail'] == pixels
    assert plan['image_grid'] == (1, n) and plan['dtype'] == TB.COLLATE_F32
    assert plan['image_bytes'] == n * pixels * (3 + 12)
    assert [p['wide'] for p in plan['planes']] == [offset == 0, True, True]
    assert [(p['src'], p['dst'], p['bytes']) for p in plan['planes']] == planes
    assert [p['first_block'] for p in plan['planes']] == [0, 1, 2] and plan['plane_blocks'] == 2 + 3      # 20000 bytes: 3 x 8 KB
    assert plan['plane_bytes'] == 2 * (pixels + 4 * pixels + 20000)


# (h, w) -> groups, tail, workgroups a sample: the boundaries of a lane's two groups (256 lanes x 2 groups x 4 pixels a workgroup)
BOUNDARY_SHAPES = {(1, 1): (0, 1, 1), (1, 2): (0, 2, 1), (1, 3): (0, 3, 1), (32, 32): (256, 0, 1), (13, 79): (256, 3, 1),
                   (4, 257): (257, 0, 1), (32, 64): (512, 0, 1), (7, 293): (512, 3, 1), (27, 76): (513, 0, 2), (41, 100): (1025, 0, 3),
                   (3, 1367): (1025, 1, 3)}
# bytes of a plane -> its workgroups (8192 bytes each)
PLANE_WORKGROUPS = {1: 1, 15: 1, 16: 1, 17: 1, 4095: 1, 4096: 1, 4097: 1, 4111: 1, 4112: 1, 8191: 1, 8192: 1, 8193: 2, 8208: 2, 12288: 2,
                    16389: 3, 24576 + 4097: 4}


@pytest.mark.parametrize('shape', list(BOUNDARY_SHAPES), ids=lambda s: f'{s[0]}x{s[1]}')
def test_plan_at_the_group_and_workgroup_boundaries(shape):
    groups, tail, blocks = BOUNDARY_SHAPES[shape]
    for dtype in R.DTYPES:
        for n in (1, 3):
            plan = TB.collate_plan([4096 + 16384 * i for i in range(n)], shape, dtype, 1 << 20, [])
            assert (plan['groups'], plan['tail'], plan['image_grid']) == (groups, tail, (blocks, n)), (dtype, n)
            assert plan['groups'] * 4 + plan['tail'] == shape[0] * shape[1] and plan['planes'] == [] and plan['plane_blocks'] == 0


def test_plan_of_plane_records_of_several_workgroups():
    src, dst = 0x7F0000100000, 0x7F0000900000
    sizes = list(PLANE_WORKGROUPS) + list(PLANE_WORKGROUPS)[::-1]           # one-workgroup records between multi-workgroup ones, both ways
    planes = [(src + 65536 * i + (i % 3 == 1), dst + 65536 * i + 4 * (i % 3 == 2), b) for i, b in enumerate(sizes)]
    plan = TB.collate_plan([], (1, 1), 'uint8', 0, planes)
    want_first = list(range(11)) + [11, 13, 15, 17, 20] + [24, 28, 31, 33, 35] + list(range(37, 48))
    assert [p['first_block'] for p in plan['planes']] == want_first
    assert want_first == [sum(PLANE_WORKGROUPS[b] for b in sizes[:i]) for i in range(len(sizes))]
    assert plan['plane_blocks'] == 2 * sum(PLANE_WORKGROUPS.values()) == 48
    assert [p['wide'] for p in plan['planes']] == [i % 3 == 0 for i in range(len(sizes))]
    assert plan['plane_bytes'] == 2 * 2 * sum(PLANE_WORKGROUPS) and plan['image_grid'] == (1, 0)
    for nbytes, blocks in PLANE_WORKGROUPS.items():                           # each alone
        plan = TB.collate_plan([], (1, 1), 'uint8', 0, [(src, dst, nbytes)])
        assert plan['planes'][0]['first_block'] == 0 and plan['plane_blocks'] == blocks, nbytes


def test_plan_grid_grows_with_the_sample_and_refuses_bad_input():
    plan = TB.collate_plan([4096], (640, 640), 'bfloat16', 8192, [])
    assert plan['groups'] == 102400 and plan['tail'] == 0 and plan['image_grid'] == (200, 1)
    assert plan['image_bytes'] == 640 * 640 * (3 + 6)
    with pytest.raises(ValueError, match='aligned'):
        TB.collate_plan([4096], (4, 4), 'float32', 8194, [])
    with pytest.raises(ValueError, match='shape'):
        TB.collate_plan([4096], (0, 4), 'float32', 8192, [])
    with pytest.raises(ValueError, match='bytes'):
        TB.collate_plan([], (4, 4), 'uint8', 8192, [(4096, 8192, 0)])
    with pytest.raises(ValueError, match='image_dtype'):
        TB.collate_plan([4096], (4, 4), 'float64', 8192, [])


# ---- fakes: a context that records its ordering calls, arrays that are plain Python ----------------------------------------------
class FakeCtx:
    def __init__(self, device=0):
        self.device, self._h, self.calls, self._next = device, True, [], 1 << 20

    handle = property(lambda self: self._h)

    @property
    def device_pool(self):
        if not hasattr(self, '_pool'):
            self._pool = N.DevicePool(self)
        return self._pool

    def malloc(self, nbytes):
        self._next += 1 << 20
        return self._next

    def free(self, ptr):
        self.calls.append(('free', ptr))

    def wait_external(self, stream):
        self.calls.append(('wait_external', stream))

    def signal_external(self, stream):
        self.calls.append(('signal_external', stream))


def fake(ctx, shape, dtype=np.uint8, ptr=1 << 30):
    return N.DevArray(ctx, ptr, shape, dtype, 0)


def sample(ctx, side=8, core=4, down=True, image=None, host_label=False):
    def mask(s):
        return Mask(mat=fake(ctx, (s, s)))

    def score(s):
        return ScoreMap(mat=fake(ctx, (s, s), np.float32), is_prob=False)

    label = None
    if down:
        label = DownsampledLabel(shape=(side // 2, side // 2), page_char_mask=mask(core // 2), page_seal_impression_char_mask=mask(core // 2),
                                 page_char_height_score_map=score(core // 2), page_text_line_mask=mask(core // 2),
                                 page_text_line_height_score_map=score(core // 2), target_core_box=Box(up=1, down=2, left=1, right=2))
    return CroppedPage(page_image=image or Image(mat=fake(ctx, (side, side, 3))),
                       page_char_mask=Mask(mat=np.zeros((core, core), np.uint8)) if host_label else mask(core),
                       page_seal_impression_char_mask=mask(core), page_char_height_score_map=score(core), page_text_line_mask=mask(core),
                       page_text_line_height_score_map=score(core), target_core_box=Box(up=2, down=5, left=2, right=5),
                       downsampled_label=label)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_collate_refusals_before_any_device_call(monkeypatch):
    ctx, other = FakeCtx(), FakeCtx()
    monkeypatch.setattr(TB, '_current_stream', lambda device: pytest.fail('a refused collate asked for a stream'))
    monkeypatch.setattr(TB, 'collate_launch', lambda *a, **k: pytest.fail('a refused collate launched'))
    with pytest.raises(ValueError, match='non-empty'):
        TB.collate_cropped_pages([])
    with pytest.raises(ValueError, match=r'sample 1, page_image: uint8 \(6, 6, 3\) in a batch of uint8 \(8, 8, 3\)'):
        TB.collate_cropped_pages([sample(ctx), sample(ctx, side=6)])
    with pytest.raises(ValueError, match='sample 1, page_char_mask'):
        TB.collate_cropped_pages([sample(ctx), sample(ctx, core=2)])
    with pytest.raises(ValueError, match='sample 1 has no downsampled_label'):
        TB.collate_cropped_pages([sample(ctx), sample(ctx, down=False)])
    with pytest.raises(TypeError, match=r'sample 0, page_char_mask.*resident\(True\)'):
        TB.collate_cropped_pages([sample(ctx, host_label=True)])
    with pytest.raises(TypeError, match=r'sample 0, page_image.*resident\(True\)'):
        TB.collate_cropped_pages([sample(ctx, image=Image(mat=np.zeros((8, 8, 3), np.uint8)))])
    with pytest.raises(ValueError, match='std has a zero'):
        TB.collate_cropped_pages([sample(ctx)], std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError, match='finite'):
        TB.collate_cropped_pages([sample(ctx)], mean=(0.2, float('nan'), 0.2))
    # constants that are finite as given and not as float32: s = 1 / (255 std) overflows, so does m = 255 mean
    with pytest.raises(ValueError, match=r'std\[0\] = 1e-41.*not finite'):
        TB.collate_cropped_pages([sample(ctx)], std=(1e-41, 1, 1))
    with pytest.raises(ValueError, match=r'std\[0\] = 1e-320.*not finite'):
        TB.collate_cropped_pages([sample(ctx)], std=(1e-320, 1, 1))
    with pytest.raises(ValueError, match=r'mean\[0\] = 2e\+36.*not finite'):
        TB.collate_cropped_pages([sample(ctx)], mean=(2e36, 0, 0))
    for bad in ('float64', torch.int8, np.int16):
        with pytest.raises(ValueError, match='image_dtype'):
            TB.collate_cropped_pages([sample(ctx)], image_dtype=bad)
    with pytest.raises(ValueError, match='one context'):
        TB.collate_cropped_pages([sample(ctx), sample(other)])
    with pytest.raises(ValueError, match=r"page_image is uint8 \(h, w, 3\)"):
        TB.collate_cropped_pages([sample(ctx, image=Image(mat=fake(ctx, (8, 8, 4))))])
    # a sample without the label is fine once it is not asked for; then `out` is checked: a missing key, a wrong shape, the wrong device
    no_down = [sample(ctx, down=False)]
    with pytest.raises(ValueError, match="out has no tensor 'page_image'"):
        TB.collate_cropped_pages(no_down, downsampled=False, out={})
    out = {'page_image': torch.empty((1, 3, 8, 8), dtype=torch.float32)}
    with pytest.raises(ValueError, match=r"out\['page_image'\] is torch.float32 \(1, 3, 8, 8\) on cpu"):
        TB.collate_cropped_pages(no_down, downsampled=False, out=out)


def test_every_image_dtype_spelling_is_understood():
    for name, t in TORCH_DTYPES.items():
        assert TB._dtype_name(name) == TB._dtype_name(t) == name
    assert TB._dtype_name(np.float16) == TB._dtype_name(np.dtype('float16')) == 'float16'


def test_as_tensor_refuses_host_backed_elements():
    for element in (Image(mat=np.zeros((4, 4, 3), np.uint8)), Mask(mat=np.zeros((4, 4), np.uint8)),
                    ScoreMap(mat=np.zeros((4, 4), np.float32)), np.zeros(3)):
        with pytest.raises(TypeError, match=r'resident\(True\)'):
            TB.as_tensor(element)
    with pytest.raises(TypeError, match='expected a DevArray'):
        TB.as_tensor('page')


class FakeTensor:
    """What from_tensor asks of a tensor, for a device this machine does not have."""

    def __init__(self, shape=(4, 5, 3), dtype=torch.uint8, contiguous=True, cuda=True, index=0):
        self.shape, self.dtype, self.is_cuda, self._contiguous = torch.Size(shape), dtype, cuda, contiguous
        self.device = SimpleNamespace(index=index)

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return 0x7F0000200000


def test_from_tensor_refusals_queue_nothing(monkeypatch):
    ctx = FakeCtx(device=0)
    monkeypatch.setattr(TB, '_current_stream', lambda device: pytest.fail('a refused tensor asked for a stream'))
    with pytest.raises(TypeError, match='uint8 or float32'):
        TB.from_tensor(torch.zeros((4, 4), dtype=torch.float64), ctx)
    with pytest.raises(TypeError, match='uint8 or float32'):
        TB.from_tensor(FakeTensor(dtype=torch.float16), ctx)
    with pytest.raises(ValueError, match='contiguous'):
        TB.from_tensor(torch.zeros((4, 6), dtype=torch.uint8)[:, ::2], ctx)
    with pytest.raises(ValueError, match='CUDA/HIP'):
        TB.from_tensor(torch.zeros((4, 4), dtype=torch.uint8), ctx)
    with pytest.raises(ValueError, match='device 0'):
        TB.from_tensor(FakeTensor(index=1), ctx)
    with pytest.raises(TypeError, match='torch.Tensor'):
        TB.from_tensor(np.zeros(3), ctx)
    assert ctx.calls == []


# ---- the array interface ------------------------------------------------------------------------------------------------------
def test_array_interface_of_a_fake_array():
    a = N.DevArray(None, 0x7F0000001000, (5, 7, 3), np.uint8, 0)
    assert a.__cuda_array_interface__ == {'shape': (5, 7, 3), 'typestr': '|u1', 'data': (0x7F0000001000, False), 'version': 2,
                                          'strides': None}
    f = N.DevArray(None, 0x7F0000002000, (4, 6), np.float32, 0)
    assert f.__cuda_array_interface__['typestr'] == '<f4' and f.__cuda_array_interface__['shape'] == (4, 6)
    v = N.DevView(f, 32, (2, 3), np.float32)                         # a view: its own address, its own shape
    assert v.__cuda_array_interface__['data'] == (0x7F0000002020, False) and v.__cuda_array_interface__['shape'] == (2, 3)
    assert np.dtype(v.__cuda_array_interface__['typestr']) == np.float32


# ---- the bookkeeping of views and borrowed tensors --------------------------------------------------------------------------------
def test_release_orders_the_pool_behind_the_viewing_streams():
    ctx = FakeCtx()
    pool = ctx.device_pool
    arr, plain = pool.empty((16, 16)), pool.empty((16, 16))
    ptr, plain_ptr = arr.ptr, plain.ptr
    TB._note_view(arr, 0x50)
    TB._note_view(arr, 0)                                              # torch's default stream has handle 0
    assert arr._viewed == {0, 0x50} and plain._viewed is None
    del plain
    gc.collect()
    assert ctx.calls == [] and pool._free[pool.GRANULE] == [plain_ptr]   # an array nobody viewed goes back as it always did
    seen = []
    ctx.wait_external = lambda stream: seen.append((stream, ptr in pool._free[pool.GRANULE]))
    del arr
    gc.collect()
    assert seen == [(0, False), (0x50, False)]                         # both waits are queued BEFORE the block can be handed out
    assert sorted(pool._free[pool.GRANULE]) == sorted([plain_ptr, ptr]) and pool._viewed == {}
    again = pool.empty((16, 16))                                       # the next owner of the block starts clean
    assert again._viewed is None


def test_a_view_of_a_view_records_on_the_block_and_later_views_inherit():
    ctx = FakeCtx()
    block = ctx.device_pool.empty((64,))
    inner = N.DevView(N.DevView(block, 8, (32,)), 4, (8,))
    TB._note_view(inner, 0x77)
    assert block._viewed == {0x77} and inner._viewed is block._viewed and inner.base._viewed is block._viewed
    assert N.DevView(block, 0, (4,))._viewed is block._viewed            # made after the view: reads wait too
    inner.after_views()
    assert ctx.calls == [('wait_external', 0x77)]
    other = FakeCtx()
    block.after_views(other)                                             # a call on another context orders that context
    assert other.calls == [('wait_external', 0x77)]


def test_as_tensor_signals_then_views(monkeypatch):
    ctx = FakeCtx(device=3)
    arr = ctx.device_pool.empty((4, 4, 3))
    arr._host = 'stale'
    order = []
    monkeypatch.setattr(TB, '_current_stream', lambda device: order.append(('stream of', device)) or 0x99)
    fake_torch = SimpleNamespace(as_tensor=lambda a, device: order.append(('as_tensor', a, device, list(ctx.calls))) or 'tensor')
    monkeypatch.setattr(TB, '_torch', lambda: fake_torch)
    assert TB.as_tensor(Image(mat=arr)) == 'tensor'
    assert order == [('stream of', 3), ('as_tensor', arr, 'cuda:3', [('signal_external', 0x99)])]
    assert arr._viewed == {0x99} and arr._host is None


def test_borrowed_tensor_orders_both_ways(monkeypatch):
    ctx = FakeCtx()
    streams = [0x11, 0x22] + [0x33] * 4
    monkeypatch.setattr(TB, '_current_stream', lambda device: streams.pop(0))
    t = FakeTensor(shape=(16, 20, 3))
    arr = TB.from_tensor(t, ctx)
    assert isinstance(arr, N.DevArray) and (arr.ptr, arr.shape, arr.dtype, arr._size) == (t.data_ptr(), (16, 20, 3), np.uint8, 0)
    assert arr.tensor is t and Image(mat=arr).on_device                  # holds the tensor; the elements take it as mat
    assert ctx.calls == [('wait_external', 0x11)]                        # wrap: the context after torch
    TB.release(arr)
    assert ctx.calls[1:] == [('signal_external', 0x22)]                  # release: torch after the context
    TB.release(arr)
    del arr
    gc.collect()
    assert len(ctx.calls) == 2                                           # once
    assert TB.from_tensor(FakeTensor(dtype=torch.float32, shape=(4, 4)), ctx).dtype == np.float32
    with pytest.raises(TypeError):
        TB.release(fake(ctx, (2, 2)))


def test_an_unreleased_borrowed_array_gives_back_when_it_dies(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(TB, '_current_stream', lambda device: 0x44)
    arr = TB.from_tensor(FakeTensor(), ctx)
    del arr
    gc.collect()
    assert ctx.calls == [('wait_external', 0x44), ('signal_external', 0x44)]
    assert ctx.device_pool._free == {}                                   # the block never enters the pool


# ---- the package ------------------------------------------------------------------------------------------------------------
def test_importing_the_package_does_not_import_torch():
    code = ("import sys; import vkit_amd; import vkit_amd.torch_bridge; import vkit_amd.pipeline.text_detection; "
            "assert 'torch' not in sys.modules, 'torch was imported'; print('ok')")
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and proc.stdout.strip() == 'ok', proc.stderr


NEW_SYMBOLS = ('vkx_ctx_wait_external', 'vkx_ctx_signal_external', 'vkx_collate_dev')


def test_new_symbols_are_declared_bound_and_exported():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vkx.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in N.EXPORTED_SYMBOLS
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = ctypes.CDLL(N.LIB_PATH)
    assert [n for n in NEW_SYMBOLS if not hasattr(handle, n)] == []
    assert (ctypes.sizeof(N.VkxCollateImage), ctypes.sizeof(N.VkxCollatePlane), ctypes.sizeof(N.VkxCollateNorm)) == (8, 24, 48)
