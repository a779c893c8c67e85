#!/usr/bin/env python3
"""Soak of the batch collate (csrc/collate.hip: k_collate_images, k_collate_planes) through vkx_collate_dev: random batches whose
pixel counts sit around the multiples of a lane's group run (1024) and plane records whose sizes sit around the multiples of half a
workgroup (4096), sources and destinations at random byte alignments, every output dtype, both layouts, the default constants and
the four edge sets of tests/collate_restate.py -- against that restatement, bit for bit, every output between canaries.
Usage: tools/soak11.py <seconds> <seed>"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch  # noqa: F401  (the restatement's bfloat16; imported here so that the budget is spent on calls)
from numpy.random import default_rng

import collate_restate as R
from vkit_amd import _native as N
from vkit_amd import torch_bridge as TB

CANARY = 0xA5
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
ctx, lib = N.default_ctx(), N.lib()
CONSTANTS = [(R.MEAN, R.STD)] + list(R.EDGE_CONSTANTS.values())


def near(step, top, spread):
    """A size within +-spread of a multiple of ``step`` up to ``top``, at least 1."""
    return max(1, step * int(rng.integers(1, top // step + 1)) + int(rng.integers(-spread, spread + 1)))


def image_shape():
    if rng.random() < 0.5:
        pixels = near(1024, 6144, 5)
        heights = [h for h in range(1, 65) if pixels % h == 0]
        h = int(rng.choice(heights))
        return h, pixels // h
    return int(rng.integers(1, 40)), int(rng.integers(1, 40))


t0 = time.time()
n_calls = n_bad = image_elements = plane_bytes = 0
while n_calls == 0 or time.time() - t0 < budget:
    n = int(rng.integers(1, 7))
    h, w = image_shape()
    dtype = R.DTYPES[int(rng.integers(4))]
    channels_first = bool(rng.integers(2))
    mean, std = CONSTANTS[int(rng.integers(len(CONSTANTS)))]
    m, s = TB.norm_constants(mean, std)
    # the sources: one buffer, image i at a byte offset of its own in 0 .. 15
    slot = (h * w * 3 + 15 + 15) // 16 * 16
    raw = rng.integers(0, 256, (n * slot,), dtype=np.uint8)
    offsets = [i * slot + int(rng.integers(0, 16)) for i in range(n)]
    images = [raw[o:o + h * w * 3].reshape(h, w, 3) for o in offsets]
    want_image = R.bits(R.collate_images(images, dtype, mean, std, channels_first=channels_first)).view(np.uint8).reshape(-1)
    # the planes: 0 .. 40 records at random alignments, half of them around the multiples of 4096
    records, src_at, dst_at, sp, dp = [], [], [], 16, 48 + (want_image.size + 15) // 16 * 16 + 48
    for _ in range(int(rng.integers(0, 41))):
        nbytes = near(4096, 40960, 17) if rng.random() < 0.5 else int(rng.integers(1, 200))
        aligned = rng.random() < 0.4
        s_mod, d_mod = (0, 0) if aligned else (int(rng.integers(0, 16)), int(rng.integers(0, 16)))
        records.append(nbytes)
        src_at.append(sp + s_mod)
        dst_at.append(dp + d_mod)
        sp = (sp + s_mod + nbytes + 15) // 16 * 16 + 16
        dp = (dp + d_mod + nbytes + 15) // 16 * 16 + 32
    plane_source = rng.integers(0, 256, (sp,), dtype=np.uint8)
    plane_source[plane_source == CANARY] = 0x5A
    want = np.full((dp + 16,), CANARY, np.uint8)
    want[48:48 + want_image.size] = want_image
    for nbytes, sa, da in zip(records, src_at, dst_at):
        want[da:da + nbytes] = plane_source[sa:sa + nbytes]

    blocks = [ctx.malloc(a.nbytes) for a in (raw, plane_source, want)]
    d_raw, d_planes, d_out = blocks
    ctx.upload(d_raw, raw)
    ctx.upload(d_planes, plane_source)
    ctx.upload(d_out, np.full_like(want, CANARY))
    assert d_out % 16 == 0 and d_planes % 16 == 0
    image_table = (N.VkxCollateImage * n)()
    for rec, o in zip(image_table, offsets):
        rec.src = d_raw + o
    plane_table = (N.VkxCollatePlane * max(1, len(records)))()
    for rec, nbytes, sa, da in zip(plane_table, records, src_at, dst_at):
        rec.src, rec.dst, rec.bytes = d_planes + sa, d_out + da, nbytes
    norm = N.VkxCollateNorm()
    norm.dst, norm.height, norm.width, norm.dtype, norm.channels_first = d_out + 48, h, w, TB._DTYPE_CODES[dtype], int(channels_first)
    norm.mean[:], norm.scale[:] = [float(v) for v in m], [float(v) for v in s]
    N.check(lib.vkx_collate_dev(ctx.handle, image_table, n, plane_table if records else None, len(records), ctypes.byref(norm)))
    ctx.sync()
    got = ctx.download(d_out, np.empty_like(want))
    ctx.sync()
    for d in blocks:
        ctx.free(d)
    n_calls += 1
    image_elements += n * h * w * 3
    plane_bytes += sum(records)
    wrong = np.flatnonzero(got != want)
    if wrong.size:
        n_bad += 1
        where = 'image batch' if 48 <= wrong[0] < 48 + want_image.size else 'planes or canaries'
        print('MISMATCH', dict(call=n_calls, n=n, shape=(h, w), dtype=dtype, channels_first=channels_first, mean=mean, std=std,
                               offsets=[o % slot for o in offsets], records=records, bytes_wrong=int(wrong.size),
                               first=int(wrong[0]), where=where), flush=True)
        break
print(json.dumps({'soak11': 'ok' if n_bad == 0 else 'MISMATCH', 'calls': n_calls, 'image_elements': image_elements,
                  'plane_bytes': plane_bytes}))
sys.exit(1 if n_bad else 0)
