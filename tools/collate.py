#!/usr/bin/env python3
"""Times three ways from a batch of device-resident CroppedPages to the batch tensors of a training loop.

    python tools/collate.py [--batch 64] [--core 512] [--pad 64] [--seconds 0.5] [--repeats 5] [--out FILE]

tools/page_steps.py fixes no crop size for PageCroppingStep, so the default is core 512, pad 64: 640 x 640 crops, 512 x 512 labels
and their 256 x 256 shrunk forms (three uint8 masks and two float32 maps each).  The samples are made once, from seeded planes.

  ``fused``         torch_bridge.collate_cropped_pages: two launches of csrc/collate.hip (and ``fused_out``: the same into the
                    tensors of the call before, ``out=``);
  ``torch_views``   torch ops on the zero-copy views: torch_bridge.as_tensor of every plane, torch.stack, and for the image
                    permute -> to(dtype, contiguous) -> sub -> mul;
  ``host``          what the library offered before the bridge: DevArray.host() of every plane (the cached copy dropped first, so
                    every call downloads), numpy stack and normalise, torch.from_numpy(...).to(device).

For float32 and bfloat16, channels first.  The three are compared before anything is timed: float32 bit for bit; bfloat16 of
``torch_views`` converts BEFORE it normalises (the chain as a user writes it) and is only checked to be close.  A call is timed with
a pair of torch events on torch's current stream around it (the collate orders that stream behind its kernels) and, beside it,
with the host clock around the call and the event's synchronise; the ways alternate inside every repeat, a point is at least
``--seconds`` of calls, and the spread is the list of the repeats.  The kernels' own time comes from the context's timing table in a
pass of its own; ``hbm_share`` is the bytes the collate has to move (3 + 3 x itemsize a pixel, a label byte in and out) over that time,
against the 8.0 TB/s of the data sheet and the 6.29 TB/s a float4 copy reaches.  Writes one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def make_samples(N, batch, core, pad, factor=2):
    from vkit_amd.element import Box, Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection.page_cropping import CroppedPage, DownsampledLabel
    from vkit_amd.torch_bridge import CROPPED_PAGE_LABELS
    ctx = N.default_ctx()
    rng = np.random.default_rng(17)
    crop, small = core + 2 * pad, core // factor

    def label(name, side):
        if name.endswith('score_map'):
            return ScoreMap(mat=ctx.to_device(rng.random((side, side), dtype=np.float32)), is_prob=False)
        return Mask(mat=ctx.to_device(rng.integers(0, 2, (side, side), dtype=np.uint8)))

    samples = []
    for _ in range(batch):
        down = DownsampledLabel(shape=(crop // factor, crop // factor), **{n: label(n, small) for n in CROPPED_PAGE_LABELS},
                                target_core_box=Box(up=pad // factor, down=pad // factor + small - 1, left=pad // factor,
                                                    right=pad // factor + small - 1))
        samples.append(CroppedPage(page_image=Image(mat=ctx.to_device(rng.integers(0, 256, (crop, crop, 3), dtype=np.uint8))),
                                   **{n: label(n, core) for n in CROPPED_PAGE_LABELS},
                                   target_core_box=Box(up=pad, down=pad + core - 1, left=pad, right=pad + core - 1),
                                   downsampled_label=down))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--core', type=int, default=512)
    ap.add_argument('--pad', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'collate_kernels.json'))
    args = ap.parse_args()

    import torch
    from vkit_amd import _native as N
    from vkit_amd import torch_bridge as TB
    import collate_restate as R
    ctx = N.default_ctx()
    device = torch.device('cuda', ctx.device)
    samples = make_samples(N, args.batch, args.core, args.pad)
    labels = TB.CROPPED_PAGE_LABELS
    fields = [(n, lambda s, n=n: getattr(s, n)) for n in labels] + \
             [('downsampled_' + n, lambda s, n=n: getattr(s.downsampled_label, n)) for n in labels]
    m_np, s_np = TB.norm_constants(R.MEAN, R.STD)

    def fused(dtype, out=None):
        return TB.collate_cropped_pages(samples, image_dtype=dtype, out=out)

    def torch_views(dtype):
        tdtype = getattr(torch, dtype)
        m = torch.from_numpy(m_np).to(device).to(tdtype).view(1, 3, 1, 1)
        s = torch.from_numpy(s_np).to(device).to(tdtype).view(1, 3, 1, 1)
        image = torch.stack([TB.as_tensor(p.page_image) for p in samples]).permute(0, 3, 1, 2)
        out = {'page_image': image.to(tdtype, memory_format=torch.contiguous_format).sub(m).mul(s)}
        for name, get in fields:
            out[name] = torch.stack([TB.as_tensor(get(p)) for p in samples])
        return out

    def host(dtype):
        def plane(element):
            element.arr.invalidate_host()
            return element.arr.host()
        image = np.stack([plane(p.page_image) for p in samples]).transpose(0, 3, 1, 2)
        image = np.ascontiguousarray((image.astype(np.float32) - m_np.reshape(1, 3, 1, 1)) * s_np.reshape(1, 3, 1, 1))
        out = {'page_image': torch.from_numpy(image).to(device).to(getattr(torch, dtype))}
        for name, get in fields:
            out[name] = torch.from_numpy(np.stack([plane(get(p)) for p in samples])).to(device)
        return out

    result = {'batch': args.batch, 'crop': args.core + 2 * args.pad, 'core': args.core, 'label_planes_per_sample': 2 * len(labels),
              'seconds_per_point': args.seconds, 'repeats': args.repeats, 'points': {}}
    for dtype in ('float32', 'bfloat16'):
        outs = fused(dtype)
        ways = {'fused': lambda: fused(dtype), 'fused_out': lambda: fused(dtype, outs), 'torch_views': lambda: torch_views(dtype),
                'host': lambda: host(dtype)}
        # the same tensors, before anything is timed
        got = {key: fn() for key, fn in ways.items()}
        torch.cuda.synchronize()
        for key in ('fused_out', 'torch_views', 'host'):
            for name in ['page_image'] + [f[0] for f in fields]:
                a, b = got['fused'][name], got[key][name]
                assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous(), (key, name)
                if name == 'page_image' and dtype == 'bfloat16' and key == 'torch_views':
                    assert float((a.float() - b.float()).abs().max()) < 0.1, (key, name)      # normalised in bfloat16: close only
                else:
                    assert R.same_bits(a, b), (key, name)
        del got

        def one_call(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop), (time.perf_counter() - t0) * 1e3

        windows = {key: {'event_ms': [], 'host_clock_ms': [], 'calls': []} for key in ways}
        for _ in range(args.repeats):                        # the ways alternate inside every repeat
            for key, fn in ways.items():
                fn()
                torch.cuda.synchronize()
                ev, wall, calls, t_end = 0.0, 0.0, 0, time.perf_counter() + args.seconds
                while time.perf_counter() < t_end or calls < 3:
                    e, w = one_call(fn)
                    ev, wall, calls = ev + e, wall + w, calls + 1
                windows[key]['event_ms'].append(round(ev / calls, 4))
                windows[key]['host_clock_ms'].append(round(wall / calls, 4))
                windows[key]['calls'].append(calls)
        for key, w in windows.items():
            w['event_ms_median'] = float(np.median(w['event_ms']))
            w['event_ms_spread'] = round(max(w['event_ms']) - min(w['event_ms']), 4)

        # the kernels alone: the context's timing table, a pass of its own
        ctx.sync()
        ctx.set_timing(1)
        ctx.reset_timings()
        calls = 50
        for _ in range(calls):
            fused(dtype, outs)
        timings = ctx.timings()
        ctx.set_timing(0)
        kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_call': n / calls} for name, (ms, n) in sorted(timings.items())}
        itemsize = 4 if dtype == 'float32' else 2
        crop = args.core + 2 * args.pad
        image_bytes = args.batch * crop * crop * 3 * (1 + itemsize)
        plane_bytes = 2 * sum(int(np.prod(outs[f[0]].shape)) * outs[f[0]].element_size() for f in fields)
        kernel_s = sum(ms for ms, _ in timings.values()) * 1e-3 / calls
        point = {'ways': windows, 'kernels': kernels, 'bytes_to_move': {'images': image_bytes, 'planes': plane_bytes},
                 'kernel_us_per_call': round(kernel_s * 1e6, 2),
                 'hbm_share': {'of_8.0_TB/s_spec': round((image_bytes + plane_bytes) / kernel_s / HBM_SPEC, 4),
                               'of_6.29_TB/s_copy': round((image_bytes + plane_bytes) / kernel_s / HBM_COPY, 4)}}
        if 'k_collate_images' in timings:
            ms, n = timings['k_collate_images']
            point['hbm_share']['image_kernel_of_8.0_TB/s_spec'] = round(image_bytes / (ms * 1e-3 / n) / HBM_SPEC, 4)
        result['points'][dtype] = point
        del outs

    result['note'] = ('event_ms: torch events on the current stream around one call, mean of a window, one entry a repeat (the ways '
                      'alternate inside a repeat); spread = max - min of the repeats; host: every call downloads (the cached host '
                      'copies are dropped first); torch_views in bfloat16 normalises in bfloat16 and is not bit-equal to the others')
    result['vkx_version'] = N.lib().vkx_version()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
