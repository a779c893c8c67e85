#!/usr/bin/env python3
"""Wall time of host-pointer entry points on dense PAGEABLE numpy planes, through the C ABI (no Python wrapper, no pinned pool):
the seven host forms that stage through vkx_host_stage.h since they left their hand-rolled copies, and three controls that always
did.  One library per process: VKX_LIB selects it, so the same script measures two builds.  Not a test.

  median wall time per call after warm-up, at 1024^2 and 2048^2
Usage: [VKX_LIB=path/to/libvkx.so] tools/host_stage_ab.py [out.json] [--reps N]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

MOVED = ('vkx_ellipse_mask_u8', 'vkx_ellipse_streak_u8', 'vkx_paint_polys', 'vkx_fill_poly_mask_u8', 'vkx_sum_f32_u8',
         'vkx_noise_normal_i16', 'vkx_np_poisson_u8')
CONTROLS = ('vkx_gaussian_blur_u8', 'vkx_resize_u8', 'vkx_fill_u8')


def calls(N, S):
    """name -> a closure that makes one host call on planes of S x S"""
    L, H, p = N.lib(), N.default_ctx().handle, N._ptr
    rng = np.random.default_rng(S)
    rgb = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    rgb_out = np.empty_like(rgb)
    gray = rng.integers(0, 48, (S, S), dtype=np.uint8)
    gray_out = np.empty_like(gray)
    mask = np.zeros((S, S), np.uint8)
    score = np.zeros((S, S), np.float32)
    i16 = np.empty((S, S, 3), np.int16)
    half = np.empty((S // 2, S // 2, 3), np.uint8)
    axes = np.array([[S // 4, S // 6], [S // 3, S // 4], [S // 8, S // 3]], np.int32)
    col = np.array([10, 200, 30, 40], np.uint8)
    pts = np.array([[S // 8, S // 10], [S - S // 8, S // 6], [S - S // 5, S - S // 7], [S // 2, S - S // 9], [S // 9, S // 2]], np.int32)
    offs = np.array([0, len(pts)], np.int32)
    vals = np.array([2.5], np.float32)
    chans = np.array([0, 1, 2], np.int32)
    sums = np.zeros(3, np.float32)
    state = (ctypes.c_uint64 * 2)(0x9E3779B97F4A7C15, 0x0123456789ABCDEF)
    inc = (ctypes.c_uint64 * 2)(0xDA3E39CB94B95BDB, 0x5851F42D4C957F2D)
    consumed, flags = ctypes.c_longlong(0), ctypes.c_uint(0)
    layer_mask = (rng.random((S // 2, S // 2)) < 0.5).astype(np.uint8)
    layer_value = rng.integers(0, 256, (S // 2, S // 2, 3), dtype=np.uint8)
    layers = (N.VkxLayer * 1)()
    lay = layers[0]
    lay.up, lay.left, lay.height, lay.width = S // 4, S // 4, S // 2, S // 2
    lay.mask, lay.mask_stride = layer_mask.ctypes.data, S // 2
    lay.alpha_scalar = 0.6
    lay.value, lay.value_stride = layer_value.ctypes.data, (S // 2) * 3
    keep = (layer_mask, layer_value)                       # the layer holds raw pointers
    return {
        'vkx_ellipse_mask_u8': lambda: L.vkx_ellipse_mask_u8(H, p(mask), S, S, S, S // 2, S // 2, p(axes), len(axes), 3),
        'vkx_ellipse_streak_u8': lambda: L.vkx_ellipse_streak_u8(H, p(rgb), S, S, 3, S * 3, S // 2, S // 2, p(axes), len(axes), 2, p(col), 0.7),
        'vkx_paint_polys': lambda: L.vkx_paint_polys(H, p(pts), p(offs), 1, p(vals), p(mask), S, p(score), S, S, S),
        'vkx_fill_poly_mask_u8': lambda: L.vkx_fill_poly_mask_u8(H, p(pts), len(pts), p(mask), S, S, S),
        'vkx_sum_f32_u8': lambda: L.vkx_sum_f32_u8(H, p(rgb), S, S, 3, S * 3, p(chans), 3, 0, p(sums)),
        'vkx_noise_normal_i16': lambda: L.vkx_noise_normal_i16(H, p(i16), S * 3, S, S, 3, 10.0, 5),
        'vkx_np_poisson_u8': lambda: L.vkx_np_poisson_u8(H, state, inc, p(gray), S * S, p(gray_out), ctypes.byref(consumed), ctypes.byref(flags)),
        'vkx_gaussian_blur_u8': lambda: L.vkx_gaussian_blur_u8(H, p(rgb), S, S, 3, S * 3, 5, 1.0, p(rgb_out), S * 3),
        'vkx_resize_u8': lambda: L.vkx_resize_u8(H, p(rgb), S, S, 3, S * 3, p(half), S // 2, S // 2, (S // 2) * 3, 1),
        'vkx_fill_u8': lambda: (keep, L.vkx_fill_u8(H, p(rgb), S, S, 3, S * 3, layers, 1))[1],
    }


def measure(reps=30, warmup=5):
    from vkit_amd import _native as N
    out = {'lib': os.path.abspath(N.LIB_PATH), 'reps': reps, 'warmup': warmup, 'unit': 'ms, median wall time per call', 'ms': {}}
    for S in (1024, 2048):
        for name, call in calls(N, S).items():
            for _ in range(warmup):
                N.check(call())
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                rc = call()
                times.append(time.perf_counter() - t0)
                N.check(rc)
            out['ms'][f'{name} {S}'] = round(float(np.median(times)) * 1e3, 4)
    return out


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    reps = int(sys.argv[sys.argv.index('--reps') + 1]) if '--reps' in sys.argv else 30
    if '--reps' in sys.argv:
        args = [a for a in args if a != str(reps)]
    result = measure(reps)
    text = json.dumps(result, indent=1)
    print(text)
    if args:
        with open(args[0], 'w') as f:
            f.write(text + '\n')
