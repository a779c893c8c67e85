#!/usr/bin/env python3
"""Times the device JPEG encoder against the raw copy-out it replaces (and against Pillow where one is installed).

    python tools/jpeg_encode.py [--quality 75] [--seconds 0.5] [--repeats 5] [--out FILE]

Two workloads at quality 75: 64 RGB crops of 640 x 640 (what tools/collate.py batches) and one 2048 x 2048 RGB page, both
device-resident and made from seeded planes: a smooth field with text-like dark strokes and a little noise, so that the
compressed size is of the order a rendered page has (pure noise would measure the worst case of the coder only).

  ``encode``    _native.jpeg_encode of the DevArrays: eight launches, one synchronisation to read the sizes, one copy of exactly
                the files' bytes -> a list of bytes;
  ``raw_host``  what the library offered before: DevArray.host() of the same pixels (the cached copy dropped first, so every call
                downloads);
  ``pillow``    where Pillow is importable: Image.fromarray(host copy).save(BytesIO, 'JPEG', quality) on ONE thread, the host
                copies already made -- what follows raw_host on the CPU.

The ways alternate inside every repeat; a point is at least ``--seconds`` of calls timed with the host clock around calls that end
in a synchronisation, after a warm-up call of every way; the spread is the list of the repeats.  The kernels' own times come from
the context's timing table (vkx_ctx_collect_timings) in a pass of its own.  Before anything is timed the device's files are
compared with Pillow's, where there is one.  Writes one JSON object."""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def page(rng, h, w):
    """a page-like RGB plane: smooth paper, dark strokes on a text grid, sensor-like noise"""
    yy, xx = np.indices((h, w))
    paper = 215 + 25 * np.sin(yy / 97.0) * np.cos(xx / 131.0)
    strokes = ((yy % 24 < 12) & (rng.random((h // 4 + 1, w // 2 + 1)).repeat(4, 0).repeat(2, 1)[:h, :w] < 0.35))
    grey = np.where(strokes, 40.0, paper) + rng.normal(0, 3, (h, w))
    tint = np.array([1.0, 0.97, 0.9])
    return np.clip(grey[..., None] * tint, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quality', type=int, default=75)
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_encode_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    try:
        from PIL import Image as PILImage
    except ImportError:
        PILImage = None
    ctx = N.default_ctx()
    rng = np.random.default_rng(23)
    workloads = {'64_crops_640x640': [page(rng, 640, 640) for _ in range(64)], '1_page_2048x2048': [page(rng, 2048, 2048)]}
    result = {'quality': args.quality, 'seconds_per_point': args.seconds, 'repeats': args.repeats, 'workloads': {}}

    for name, mats in workloads.items():
        devs = [ctx.to_device(m) for m in mats]

        def encode():
            return N.jpeg_encode(devs, quality=args.quality)

        def raw_host():
            for d in devs:
                d.invalidate_host()
            return [d.host() for d in devs]

        def pillow():
            out = []
            for m in mats:
                buf = io.BytesIO()
                PILImage.fromarray(m).save(buf, format='JPEG', quality=args.quality)
                out.append(buf.getvalue())
            return out

        ways = {'encode': encode, 'raw_host': raw_host}
        if PILImage is not None:
            ways['pillow'] = pillow
        files = encode()
        point = {'images': len(mats), 'raw_bytes': int(sum(m.nbytes for m in mats)), 'jpeg_bytes': int(sum(len(f) for f in files))}
        if PILImage is not None:
            point['equal_to_pillow'] = bool(files == pillow())
        windows = {key: {'ms': [], 'calls': []} for key in ways}
        for fn in ways.values():        # warm-up: code objects, pools, page-locked blocks
            fn()
        ctx.sync()
        for _ in range(args.repeats):
            for key, fn in ways.items():
                calls, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < args.seconds or calls < 3:
                    fn()                 # every way ends in a synchronisation (or never touches the device)
                    calls += 1
                windows[key]['ms'].append(round((time.perf_counter() - t0) * 1e3 / calls, 4))
                windows[key]['calls'].append(calls)
        for w in windows.values():
            w['ms_median'] = float(np.median(w['ms']))
            w['ms_spread'] = round(max(w['ms']) - min(w['ms']), 4)
        point['ways'] = windows

        # the kernels alone: the context's timing table, a pass of its own
        ctx.sync()
        ctx.set_timing(1)
        ctx.reset_timings()
        calls = 20
        for _ in range(calls):
            encode()
        timings = ctx.timings()
        ctx.set_timing(0)
        point['kernels'] = {k: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_call': n / calls}
                            for k, (ms, n) in sorted(timings.items())}
        point['kernel_us_per_call'] = round(sum(ms for ms, _ in timings.values()) * 1e3 / calls, 2)
        result['workloads'][name] = point
        del devs

    result['note'] = ('ms: host clock around calls that end in a synchronisation, mean of a window, one entry a repeat (the ways '
                      'alternate inside a repeat); spread = max - min of the repeats; raw_host downloads on every call; pillow '
                      'encodes host copies that are already made, on one thread')
    if PILImage is not None:
        import PIL
        from PIL import features
        result['pillow'] = f'{PIL.__version__} / libjpeg-turbo {features.version_feature("libjpeg_turbo")}'
    result['vkx_version'] = N.lib().vkx_version()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
