"""The PyTorch bridge: device arrays as tensors and tensors as device arrays without a copy, and the batch collate.

What the steps produce inside ``_native.resident(True)`` are samples whose planes are ``DevArray`` s in HBM; what a training loop
wants is a batch of tensors on the same GPU.  ``DevArray.host()`` is a device-to-host copy, and the consumer's collate and
``.to(device)`` the way back; this module leaves the planes where they are.

* ``as_tensor(x)``: a ``DevArray`` / ``DevView`` or a device-backed ``Image`` / ``Mask`` / ``ScoreMap`` as a ``torch.Tensor`` on the
  same memory (``__cuda_array_interface__``, which torch-ROCm reads; the tensor holds a reference to the array).
* ``from_tensor(t)`` / ``release(a)``: a contiguous uint8 / float32 tensor as a borrowed ``DevArray`` the elements take as ``mat``.
* ``collate_cropped_pages`` / ``collate_cropped_page_text_regions``: the samples of the cropping steps into one dict of batch
  tensors, in two launches (csrc/collate.hip): the images normalised, transposed and converted on the way, the labels copied.

The library's kernels run on the context's own stream, torch's on ``torch.cuda.current_stream()``.  Nothing here waits on the host:
the two streams are ordered by events (``Context.wait_external`` / ``signal_external``) at every point where memory changes hands,
and an array remembers the streams it was viewed from (``DevArray._viewed``) so that the library orders itself behind them before it
reads the array again and before the array's block returns to the pool.

torch is imported on first use: ``import vkit_amd`` does not import it.
"""
import ctypes
import weakref

import numpy as np

from . import _native
from ._native import DevArray

# of csrc/collate.hip (the launch geometry ``collate_plan`` restates)
COLLATE_U8, COLLATE_F32, COLLATE_F16, COLLATE_BF16 = 0, 1, 2, 3
GROUP_PIXELS = 4                  # pixels of one load / one store a plane
GROUPS_PER_BLOCK = 512
PLANE_BLOCK_BYTES = 8192
_DTYPE_CODES = {'uint8': COLLATE_U8, 'float32': COLLATE_F32, 'float16': COLLATE_F16, 'bfloat16': COLLATE_BF16}
_ITEMSIZE = {'uint8': 1, 'float32': 4, 'float16': 2, 'bfloat16': 2}

CROPPED_PAGE_LABELS = ('page_char_mask', 'page_seal_impression_char_mask', 'page_char_height_score_map', 'page_text_line_mask',
                       'page_text_line_height_score_map')
CROPPED_PAGE_TEXT_REGION_LABELS = ('page_char_mask', 'page_char_height_score_map', 'page_char_gaussian_score_map',
                                   'page_char_bounding_box_mask')


def _torch():
    import torch
    return torch


def _current_stream(device):
    """The handle (an int; 0 for the default stream) of torch's current stream on ``device``."""
    return int(_torch().cuda.current_stream(device).cuda_stream)


def _device_array(x):
    """The ``DevArray`` behind ``x``, or the refusal of a host-backed one."""
    arr = x if isinstance(x, DevArray) else getattr(x, 'arr', None)
    if isinstance(arr, DevArray):
        return arr
    if isinstance(arr, np.ndarray) or isinstance(x, np.ndarray):
        raise TypeError(f'{type(x).__name__} is host-backed: only device memory can be shared without a copy; make it inside '
                        f'``with vkit_amd._native.resident(True):``')
    raise TypeError(f'expected a DevArray or a device-backed Image / Mask / ScoreMap, got {type(x).__name__}')


def _note_view(arr, stream):
    """``arr`` is handed to a user on the foreign stream ``stream``: recorded on the array, on the array it is a view of, and with
    the pool that will take the block back."""
    root = arr
    while getattr(root, 'base', None) is not None:
        root = root.base
    if root._size and root.ctx is not None:
        root.ctx.device_pool.note_view(root, stream)          # (the set is the pool's: it outlives the array)
    else:
        if root._viewed is None:
            root._viewed = set()
        root._viewed.add(stream)
    node = arr
    while node is not root:
        node._viewed = root._viewed
        node = node.base


def as_tensor(x):
    """``x`` as a ``torch.Tensor`` of the same shape and dtype on the same device memory.  torch's current stream continues after
    everything the library has queued so far, so the tensor can be used at once; the tensor keeps the array alive."""
    arr = _device_array(x)
    torch = _torch()
    ctx = arr.ctx
    stream = _current_stream(ctx.device)
    ctx.signal_external(stream)
    _note_view(arr, stream)
    arr.invalidate_host()                  # the tensor is writable: a host copy made before it would go stale unnoticed
    return torch.as_tensor(arr, device=f'cuda:{ctx.device}')


class BorrowedArray(DevArray):
    """A tensor's memory as a ``DevArray``: never in the pool, holds the tensor, and hands the memory back -- orders torch's current
    stream behind the context's -- on ``release`` or when it dies."""

    __slots__ = ('tensor', '_give_back')


def _give_back(ctx, device):
    if ctx._h:
        ctx.signal_external(_current_stream(device))


def _tensor_dtype(t):
    torch = _torch()
    return {torch.uint8: np.uint8, torch.float32: np.float32}.get(t.dtype)


def from_tensor(t, ctx=None):
    """A contiguous uint8 or float32 CUDA/HIP tensor as a borrowed ``DevArray`` of ``ctx`` (default: the thread's default context)
    that the elements and the operators take like any other.  The context's stream continues after torch's current stream."""
    if not hasattr(t, 'data_ptr'):
        raise TypeError(f'expected a torch.Tensor, got {type(t).__name__}')
    dtype = _tensor_dtype(t)
    if dtype is None:
        raise TypeError(f'from_tensor takes uint8 or float32, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError('from_tensor takes a contiguous tensor (t.contiguous() copies once)')
    if not t.is_cuda:
        raise ValueError('from_tensor takes a CUDA/HIP tensor: a CPU tensor is numpy already (t.numpy())')
    ctx = ctx or _native.default_ctx()
    if t.device.index != ctx.device:
        raise ValueError(f'the tensor is on {t.device}, the context on device {ctx.device}')
    arr = BorrowedArray(ctx, int(t.data_ptr()), tuple(t.shape), dtype, 0)
    arr.tensor = t
    ctx.wait_external(_current_stream(ctx.device))
    arr._give_back = weakref.finalize(arr, _give_back, ctx, ctx.device)
    arr._give_back.atexit = False
    return arr


def release(arr):
    """The library is done with the borrowed ``arr``: torch's current stream continues after everything the context has queued so
    far (what an unreleased array does when it dies)."""
    if not isinstance(arr, BorrowedArray):
        raise TypeError('release takes an array that from_tensor made')
    arr._give_back()


# ---- the collate ---------------------------------------------------------------------------------------------------------
def norm_constants(mean, std):
    """(m, s) of ``out = (float32(x) - m_c) * s_c``: m_c = float32(255 mean_c), s_c = float32(1 / (255 std_c)), each worked out in
    float64 and rounded once.  Both must be finite AS float32 (a std below about 1.2e-41 or a mean above about 1.3e36 is refused
    here, before anything is allocated or queued); a scale that rounds to zero is finite."""
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError('mean and std have one entry a channel (3)')
    if not all(np.isfinite(v) for v in mean + std):
        raise ValueError('mean and std are finite')
    if any(v == 0.0 for v in std):
        raise ValueError('std has a zero: the scale 1 / (255 std) does not exist')
    with np.errstate(over='ignore', divide='ignore'):
        m = np.array([255.0 * v for v in mean], np.float64).astype(np.float32)
        # (np.float64: 255 std may be subnormal, or round to zero, and its reciprocal is infinite -- refused just below)
        s = (1.0 / np.array([255.0 * v for v in std], np.float64)).astype(np.float32)
    for name, given, constants in (('mean', mean, m), ('std', std, s)):
        for c in range(3):
            if not np.isfinite(constants[c]):
                raise ValueError(f'{name}[{c}] = {given[c]!r}: its float32 constant {"255 mean" if name == "mean" else "1 / (255 std)"} '
                                 f'is not finite')
    return m, s


def _dtype_name(dtype):
    """'uint8' / 'float32' / 'float16' / 'bfloat16' of a name, a numpy dtype or a torch dtype."""
    name = dtype if isinstance(dtype, str) else str(dtype)
    name = name.replace('torch.', '').replace("<class 'numpy.", '').replace("'>", '')
    if name not in _DTYPE_CODES:
        raise ValueError(f'image_dtype {dtype!r} is not one of uint8, float32, float16, bfloat16')
    return name


def collate_plan(image_ptrs, image_shape, image_dtype, image_dst, planes):
    """What one vkx_collate_dev call is given and how csrc/collate.hip lays it out, on the host: ``image_ptrs`` the sources of shape
    ``image_shape`` = (h, w), ``image_dst`` the address of the batch, ``planes`` (src, dst, bytes) copies.  -> a dict: ``images`` the
    source addresses as given (any byte alignment: one path reads them all), ``groups`` / ``tail`` the 4-pixel groups and the
    left-over pixels of one sample, ``image_grid`` (x, y), ``image_bytes`` read + written; ``planes`` the records with ``wide`` (16
    bytes a lane: both ends 16-byte aligned; single bytes otherwise) and ``first_block``; ``plane_blocks``, ``plane_bytes``."""
    h, w = (int(v) for v in image_shape)
    name = _dtype_name(image_dtype)
    n = len(image_ptrs)
    if n and (h < 1 or w < 1):
        raise ValueError(f'an image of shape {(h, w)}')
    pixels = h * w
    groups, tail = divmod(pixels, GROUP_PIXELS)
    if n and int(image_dst) % _ITEMSIZE[name]:
        raise ValueError('the image batch is not aligned to its element')
    records, first = [], 0
    for src, dst, nbytes in planes:
        src, dst, nbytes = int(src), int(dst), int(nbytes)
        if nbytes < 1 or nbytes >= 1 << 31:
            raise ValueError(f'a plane of {nbytes} bytes')
        records.append(dict(src=src, dst=dst, bytes=nbytes, wide=(src | dst) % 16 == 0, first_block=first))
        first += -(-nbytes // PLANE_BLOCK_BYTES)
    return dict(images=[int(p) for p in image_ptrs], dtype=_DTYPE_CODES[name], groups=groups, tail=tail,
                image_grid=(max(1, -(-groups // GROUPS_PER_BLOCK)), n), image_bytes=n * pixels * 3 * (1 + _ITEMSIZE[name]),
                planes=records, plane_blocks=first, plane_bytes=2 * sum(r['bytes'] for r in records))


def collate_launch(ctx, plan, image_shape, image_dst, channels_first, mean_scale):
    """One vkx_collate_dev call from a ``collate_plan``: at most two launches on the context's stream, no synchronisation."""
    n, n_planes = len(plan['images']), len(plan['planes'])
    images = (_native.VkxCollateImage * max(n, 1))()
    for rec, ptr in zip(images, plan['images']):
        rec.src = ptr
    planes = (_native.VkxCollatePlane * max(n_planes, 1))()
    for rec, p in zip(planes, plan['planes']):
        rec.src, rec.dst, rec.bytes = p['src'], p['dst'], p['bytes']
    norm = _native.VkxCollateNorm()
    norm.dst, norm.height, norm.width = image_dst, int(image_shape[0]), int(image_shape[1])
    norm.dtype, norm.channels_first = plan['dtype'], int(bool(channels_first))
    norm.mean[:], norm.scale[:] = [float(v) for v in mean_scale[0]], [float(v) for v in mean_scale[1]]
    _native.check(_native.lib().vkx_collate_dev(ctx.handle, images if n else None, n, planes if n_planes else None, n_planes,
                                                ctypes.byref(norm) if n else None))


def _plane_of(sample, owner, name, index):
    element = getattr(owner, name)
    if element is None:
        raise ValueError(f'sample {index}: {name} is None')
    try:
        return _device_array(element)
    except TypeError as e:
        raise TypeError(f'sample {index}, {name}: {e}') from None


def _gather(samples, labels, downsampled):
    """{output name: [DevArray of every sample]} with the shapes, dtypes and contexts checked; 'page_image' first."""
    if not isinstance(samples, (list, tuple)) or len(samples) == 0:
        raise ValueError('collate takes a non-empty list of samples')
    fields = {'page_image': [_plane_of(s, s, 'page_image', i) for i, s in enumerate(samples)]}
    for name in labels:
        fields[name] = [_plane_of(s, s, name, i) for i, s in enumerate(samples)]
    if downsampled:
        for i, s in enumerate(samples):
            if s.downsampled_label is None:
                raise ValueError(f'sample {i} has no downsampled_label (the step ran without enable_downsample_labeling): collate '
                                 f'with downsampled=False')
        for name in labels:
            fields['downsampled_' + name] = [_plane_of(s, s.downsampled_label, name, i) for i, s in enumerate(samples)]
    ctx = fields['page_image'][0].ctx
    for name, arrs in fields.items():
        first = arrs[0]
        for i, a in enumerate(arrs):
            if a.ctx is not ctx:
                raise ValueError(f'sample {i}, {name}: the samples of one batch live on one context')
            if a.shape != first.shape or a.dtype != first.dtype:
                raise ValueError(f'sample {i}, {name}: {a.dtype} {a.shape} in a batch of {first.dtype} {first.shape}')
        if name == 'page_image':
            if first.dtype != np.uint8 or first.ndim != 3 or first.shape[2] != 3 or first.size == 0:
                raise ValueError(f'page_image is uint8 (h, w, 3), got {first.dtype} {first.shape}')
        elif first.dtype not in (np.uint8, np.float32) or first.ndim != 2 or first.size == 0:
            raise ValueError(f'{name} is a uint8 or float32 (h, w) plane, got {first.dtype} {first.shape}')
    return ctx, fields


def _boxes(boxes):
    return _torch().tensor([[b.up, b.down, b.left, b.right] for b in boxes], dtype=_torch().int32)


def _collate(samples, labels, passthrough, image_dtype, mean, std, channels_first, downsampled, out):
    name = _dtype_name(image_dtype)
    mean_scale = norm_constants(mean, std)
    ctx, fields = _gather(samples, labels, downsampled)
    torch = _torch()
    n = len(samples)
    h, w = fields['page_image'][0].shape[:2]
    device = torch.device('cuda', ctx.device)
    wanted = {}
    for key, arrs in fields.items():
        if key == 'page_image':
            wanted[key] = ((n, 3, h, w) if channels_first else (n, h, w, 3), getattr(torch, name))
        else:
            wanted[key] = ((n,) + arrs[0].shape, torch.uint8 if arrs[0].dtype == np.uint8 else torch.float32)
    if out is not None:
        for key, (shape, dtype) in wanted.items():
            t = out.get(key)
            if not isinstance(t, torch.Tensor):
                raise ValueError(f'out has no tensor {key!r}')
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
                raise ValueError(f'out[{key!r}] is {t.dtype} {tuple(t.shape)} on {t.device}'
                                 f'{"" if t.is_contiguous() else ", not contiguous"}; the batch needs {dtype} {shape} on {device}')
    stream = _current_stream(ctx.device)
    result = {key: (out[key] if out is not None else torch.empty(shape, dtype=dtype, device=device))
              for key, (shape, dtype) in wanted.items()}
    planes = []
    for key, arrs in fields.items():
        if key != 'page_image':
            base, nbytes = result[key].data_ptr(), arrs[0].nbytes
            planes += [(a.ptr, base + i * nbytes, nbytes) for i, a in enumerate(arrs)]
    plan = collate_plan([a.ptr for a in fields['page_image']], (h, w), name, result['page_image'].data_ptr(), planes)
    # the outputs are torch's (their last users are on its stream), the sources may have been written through a view
    ctx.wait_external(stream)
    for arrs in fields.values():
        for a in arrs:
            if a._viewed:
                a.after_views()
    collate_launch(ctx, plan, (h, w), result['page_image'].data_ptr(), channels_first, mean_scale)
    ctx.signal_external(stream)
    result['target_core_box'] = _boxes([s.target_core_box for s in samples])
    if downsampled:
        result['downsampled_target_core_box'] = _boxes([s.downsampled_label.target_core_box for s in samples])
    for key in passthrough:
        result[key] = [getattr(s, key) for s in samples]
        if downsampled:
            result['downsampled_' + key] = [getattr(s.downsampled_label, key) for s in samples]
    return result


def collate_cropped_pages(samples, *, image_dtype='float32', mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                          channels_first=True, downsampled=True, out=None):
    """The ``CroppedPage`` s of ``PageCroppingStep`` (made inside ``resident(True)``, of any number of pages) as one batch, a dict of
    tensors on their device: ``page_image`` [N, 3, S, S] (``channels_first``) or [N, S, S, 3] of ``image_dtype`` (uint8, float32,
    float16 or bfloat16, by name or as a torch dtype; the float types hold ``(x / 255 - mean) / std`` in the fixed arithmetic of
    ``norm_constants``), every label [N, h, w] under its own name and, with ``downsampled``, as ``downsampled_<name>``;
    ``target_core_box`` / ``downsampled_target_core_box`` int32 [N, 4] (up, down, left, right) on the CPU.  ``out``: the dict of an
    earlier call of the same shapes, written again instead of allocating.  Two launches on the samples' context, ordered after and
    before torch's current stream: the tensors may be used, and the samples dropped, at once."""
    return _collate(samples, CROPPED_PAGE_LABELS, (), image_dtype, mean, std, channels_first, downsampled, out)


def collate_cropped_page_text_regions(samples, *, image_dtype='float32', mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                                      channels_first=True, downsampled=True, out=None):
    """``collate_cropped_pages`` for the ``CroppedPageTextRegion`` s of ``PageTextRegionCroppingStep``;
    ``page_char_regression_labels`` (and ``downsampled_page_char_regression_labels``) pass through as the lists they are."""
    return _collate(samples, CROPPED_PAGE_TEXT_REGION_LABELS, ('page_char_regression_labels',), image_dtype, mean, std,
                    channels_first, downsampled, out)
