#!/usr/bin/env python3
"""Times char binding on a synthetic page: PageTextRegionStep.build_page_text_region_infos (csrc/polygon_overlap.hip) against the
same answers composed from what the library offered before it.

    timeout -k 10 300 python tools/char_binding.py [--page 1024] [--regions 64] [--chars 2048] [--repeats 5] [--out FILE]

The page (fixed seed): ``--regions`` slanted text-region quads in four columns, ``--chars`` char quads spread over them, every
thirteenth hanging over its region's lower edge into the region below (or off the page's regions in the last row).

  ``batched``    build_page_text_region_infos: the envelope pairs and point tables on the host, three launches, one copy-out, one
                 synchronisation;
  ``composed``   the loops of tests/char_binding_restate.py over per-polygon ``Polygon.np_mask`` (one vkx_fill_poly_mask_u8 call
                 and one synchronisation a polygon) and ``Polygon.bounding_box``, the areas and the intersections in numpy.

Both get fresh Polygon objects for every call (``np_mask`` is cached on the object), made outside the clock; the two are
compared before anything is timed.  A call is timed with the host clock (both end in a device synchronise); the ways alternate
inside every repeat; the spread is the list of the repeats.  The kernels' own time comes from the context's timing table in a
pass of its own.  Writes one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def make_page(page, n_regions, n_chars, seed=20261021):
    """-> (region point arrays, char point arrays), float64 (4, 2) each"""
    rng = np.random.default_rng(seed)
    columns = 4
    rows = (n_regions + columns - 1) // columns
    cell_w, cell_h = page // columns, page // rows
    regions, chars = [], []
    for r in range(n_regions):
        left, up = (r % columns) * cell_w + 6, (r // columns) * cell_h + 4
        w, h = cell_w - 14, max(cell_h - 10, 8)
        slant = rng.integers(-3, 4, 4)
        regions.append(np.array([(left, up + 3 + slant[0]), (left + w, up + 3 + slant[1]), (left + w, up + h - 3 + slant[2]),
                                 (left, up + h - 3 + slant[3])], np.float64))
    for k in range(n_chars):
        r = k % n_regions
        left, up = (r % columns) * cell_w + 6, (r // columns) * cell_h + 4
        w, h = cell_w - 14, max(cell_h - 10, 8)
        per = (n_chars + n_regions - 1) // n_regions
        cw = max(w // per, 4)
        x = left + (k // n_regions) * cw + rng.random() * 2
        y = up + 4 + rng.random() * 3
        if k % 13 == 0:
            y += h // 2 + 6                          # hangs over the region's lower edge, into the region below
        ch = max(h - 10, 5)
        chars.append(np.array([(x, y), (x + cw - 1 + rng.random(), y + rng.random()), (x + cw - 1, y + ch), (x + rng.random(), y + ch)],
                              np.float64))
    return regions, chars


def polygons_of(tables):
    from vkit_amd.element import Polygon
    return [Polygon.from_xy_pairs([(float(x), float(y)) for x, y in t]) for t in tables]


def composed(region_polygons, char_polygons):
    """the binding of tests/char_binding_restate.py (Case.bind) over Polygon.np_mask and Polygon.bounding_box"""
    import char_binding_restate as R

    def mask(polygon):
        box = polygon.bounding_box
        return (box.up, box.down, box.left, box.right), polygon.np_mask.astype(np.uint8)

    def envelope(polygon):
        xy = polygon.to_np_array()
        return int(xy[:, 0].min()), int(xy[:, 0].max()), int(xy[:, 1].min()), int(xy[:, 1].max())

    region_masks = [mask(p) for p in region_polygons]
    region_envelopes = [envelope(p) for p in region_polygons]
    bound = []
    for polygon in char_polygons:
        char_mask, char_envelope = None, envelope(polygon)
        best, ratio_max = None, 0
        for a, region_envelope in enumerate(region_envelopes):
            if not R.envelopes_meet(region_envelope, char_envelope):
                continue
            char_mask = char_mask or mask(polygon)
            ratio = R.intersected_ratio(region_masks[a], char_mask, True)
            if ratio > ratio_max:
                ratio_max, best = ratio, a
        bound.append(-1 if best is None else best)
    return bound


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--page', type=int, default=1024)
    ap.add_argument('--regions', type=int, default=64)
    ap.add_argument('--chars', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='batched calls a repeat, and calls of the kernel pass')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'char_binding_kernels.json'))
    args = ap.parse_args()

    import logging
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import PageTextRegionStep, intersected_polygon_ratios
    logging.getLogger('vkit_amd.pipeline.text_detection.page_text_region').setLevel(logging.ERROR)
    ctx = N.default_ctx()
    regions, chars = make_page(args.page, args.regions, args.chars)

    def batched(region_polygons, char_polygons):
        infos = PageTextRegionStep.build_page_text_region_infos(region_polygons, char_polygons)
        index = {id(p): k for k, p in enumerate(region_polygons)}
        bound = {id(p): index[id(info.precise_text_region_polygon)] for info in infos for p in info.char_polygons}
        return [bound.get(id(p), -1) for p in char_polygons]

    # the same answers, before anything is timed
    got, want = batched(polygons_of(regions), polygons_of(chars)), composed(polygons_of(regions), polygons_of(chars))
    assert got == want, 'the batched binding differs from the composed one'
    pairs, _, _, _ = intersected_polygon_ratios(polygons_of(regions), polygons_of(chars))

    def clock(fn, calls):
        total = 0.0
        for _ in range(calls):
            fresh = polygons_of(regions), polygons_of(chars)
            ctx.sync()
            t0 = time.perf_counter()
            fn(*fresh)
            total += time.perf_counter() - t0
        return round(total / calls * 1e3, 4)

    ways = {'batched': [], 'composed': []}
    for _ in range(args.repeats):                    # the ways alternate inside every repeat
        ways['batched'].append(clock(batched, args.calls))
        ways['composed'].append(clock(composed, 1))

    # the kernels alone: the context's timing table, a pass of its own
    region_polygons, char_polygons = polygons_of(regions), polygons_of(chars)
    ctx.sync()
    ctx.set_timing(1)
    ctx.reset_timings()
    for _ in range(args.calls):
        PageTextRegionStep.bind_char_polygons(region_polygons, char_polygons)
    timings = ctx.timings()
    ctx.set_timing(0)
    kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_call': n / args.calls} for name, (ms, n) in sorted(timings.items())}
    # the host half alone: everything of a call but the library call, the copy-out and the synchronisation
    from vkit_amd.pipeline.text_detection import envelope_pairs, polygon_overlap_tables
    t0 = time.perf_counter()
    for _ in range(args.calls):
        records, _, envelopes = polygon_overlap_tables(region_polygons + char_polygons)
        envelope_pairs(envelopes[:len(regions)], envelopes[len(regions):])
    host_tables_ms = round((time.perf_counter() - t0) / args.calls * 1e3, 4)

    batched_ms, composed_ms = float(np.median(ways['batched'])), float(np.median(ways['composed']))
    result = {'page': args.page, 'regions': len(regions), 'chars': len(chars), 'pairs': int(len(pairs)),
              'bound_chars': int(sum(b >= 0 for b in got)), 'repeats': args.repeats, 'batched_calls_per_repeat': args.calls,
              'wall_ms': ways, 'wall_ms_median': {'batched': batched_ms, 'composed': composed_ms},
              'composed_over_batched': round(composed_ms / batched_ms, 2), 'kernels': kernels,
              'kernel_us_per_call': round(sum(ms for ms, _ in timings.values()) * 1e3 / args.calls, 2),
              'host_tables_ms_per_call': host_tables_ms,
              'note': 'wall_ms: host clock around one call that ends in a device synchronise, mean of a window, one entry a repeat '
                      '(the ways alternate inside a repeat); composed: one vkx_fill_poly_mask_u8 call and synchronisation a polygon, '
                      'one call a repeat; host_tables_ms_per_call: polygon_overlap_tables + envelope_pairs alone',
              'vkx_version': N.lib().vkx_version()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
