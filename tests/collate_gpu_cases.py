"""What the GPU tests of the batch collate share (tests/test_gpu_torch_bridge.py, tests/test_gpu_collate_geometry.py): the modules,
samples whose planes lie at chosen addresses, and output tensors carved between canaries."""
import numpy as np

LABELS = ('page_char_mask', 'page_seal_impression_char_mask', 'page_char_height_score_map', 'page_text_line_mask',
          'page_text_line_height_score_map')
FLOAT_LABELS = ('page_char_height_score_map', 'page_text_line_height_score_map')
CANARY = 0xA5


def _mods():
    import torch
    from vkit_amd import _native as N
    from vkit_amd import torch_bridge as TB
    return torch, N, TB


def _samples(N, ctx, rng, n, shape, label_shape, first_offset):
    """n CroppedPages whose images are views at byte offsets first_offset, +1, ... (mod 4) of one buffer; the labels views and
    arrays of their own.  -> (samples, the host planes by output name)"""
    from vkit_amd.element import Box, Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection.page_cropping import CroppedPage, DownsampledLabel
    h, w = shape
    lh, lw = label_shape
    slot = (h * w * 3 + 3 + 15) // 16 * 16
    raw = rng.integers(0, 256, (n * slot,), dtype=np.uint8)
    buffer = ctx.to_device(raw)
    labels_raw = rng.integers(0, 2, (n * 5 * (lh * lw + 1),), dtype=np.uint8)
    labels_buffer = ctx.to_device(labels_raw)
    host = {'page_image': []}
    samples = []
    at = 0
    for i in range(n):
        off = i * slot + (first_offset + i) % 4
        host['page_image'].append(raw[off:off + h * w * 3].reshape(h, w, 3))
        image = Image(mat=N.DevView(buffer, off, (h, w, 3)))

        def label(name, shp, prefix=''):
            nonlocal at
            if name in FLOAT_LABELS:
                plane = (rng.random(shp, dtype=np.float32) * 3 - 1).astype(np.float32)
                element = ScoreMap(mat=ctx.to_device(plane), is_prob=False)
            elif name == 'page_text_line_mask':
                plane = rng.integers(0, 2, shp, dtype=np.uint8)           # an array of its own: 16-byte aligned
                element = Mask(mat=ctx.to_device(plane))
            else:
                size = shp[0] * shp[1]
                plane = labels_raw[at:at + size].reshape(shp)            # a view at an odd address
                element = Mask(mat=N.DevView(labels_buffer, at, shp))
                at += size + 1
            host.setdefault(prefix + name, []).append(plane)
            return element

        down_shape = (max(1, lh // 2), max(1, lw // 2))
        down = DownsampledLabel(shape=down_shape, target_core_box=Box(up=i, down=i + 1, left=1, right=2),
                                **{name: label(name, down_shape, 'downsampled_') for name in LABELS})
        samples.append(CroppedPage(page_image=image, target_core_box=Box(up=2 + i, down=5, left=3, right=6 + i), downsampled_label=down,
                                   **{name: label(name, (lh, lw)) for name in LABELS}))
    return samples, host


def _carve(torch, device, wanted):
    """Tensors of the wanted (shape, dtype) carved out of one canary-filled buffer, 48 canary bytes before and after each."""
    sizes = {k: int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size() for k, (shape, dtype) in wanted.items()}
    total = sum((s + 15) // 16 * 16 + 48 for s in sizes.values()) + 48
    buffer = torch.full((total,), CANARY, dtype=torch.uint8, device=device)
    out, used, at = {}, np.zeros(total, bool), 48
    for key, (shape, dtype) in wanted.items():
        out[key] = buffer[at:at + sizes[key]].view(dtype).view(shape)
        used[at:at + sizes[key]] = True
        at += (sizes[key] + 15) // 16 * 16 + 48
    return buffer, out, used
