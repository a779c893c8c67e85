#!/usr/bin/env python3
"""Regenerates tests/golden/text_region_cropping.npz by running THE REFERENCE's own PageTextRegionCroppingStep.run
(vkit/pipeline/text_detection/page_text_region_cropping.py) on small synthetic pages, three seeds a case.

    python tests/golden/make_text_region_cropping_golden.py

The missing third-party modules are stubbed exactly as make_golden.py stubs them (it is imported for that).  cv.resize is the
oracle's, as in make_cropping_golden.py (the step calls it with INTER_AREA for its downsampled labels).  The only other patch
replaces the three shapely names the step reaches -- STRtree, ShapelyPoint and build_shapely_polygon_as_box, all MagicMock
stubs here -- by the brute-force closed-box stand-ins below: a point intersects a box when minx <= x <= maxx and
miny <= y <= maxy, the edge included, which is shapely's definition of ``intersects``.  The stand-in tree answers in
DESCENDING order, so the reference's ``sorted`` is what orders the labels.  One stub needs a value to be usable at all: the
step hands ``rotate.distort`` its config as a mapping, which the reference structures with cattrs (a MagicMock here), so the
stub's ``structure`` builds the config class from the mapping, ``cls(**mapping)``, which is what cattrs does for a flat attrs
class.  Everything else -- the windows, the draws, the rotation of the centre, the loop, the label shifting and downsampling,
the padding and the crops -- is the reference's code running for real.

The labels are reference PageCharRegressionLabel objects built directly from random convex quads (the centroid label at the
mean of the corners, the deviate labels inside the quad), with distinct (tag, char_idx, point) keys, so that the kept labels of a
sample can be identified from the sample itself.

Stored per run, in one JSON ``index`` row: the config, the seed, the page shapes and the angle, the label tables, every Cropper
the run made (original_box, target_box, original_core_box), the generator state after ``run``, and per sample the kept label
indices (into the centroid labels and into the deviate labels), the shifted and the downsampled label points and where its
planes sit in a few flat arrays.  The page planes are stored once a case.  Data only, never reference source text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import oracle as O  # noqa: E402
from make_cropping_golden import blocky, boxes_mask  # noqa: E402
from vkit.element import Image, Mask, Point, ScoreMap  # noqa: E402
from vkit.element import box as ref_box  # noqa: E402
from vkit.mechanism import cropper as ref_cropper  # noqa: E402
from vkit.mechanism.distortion import rotate  # noqa: E402
from vkit.pipeline.text_detection import page_text_region_cropping as TC  # noqa: E402
from vkit.pipeline.text_detection import page_text_region_label as L  # noqa: E402
from vkit.pipeline.text_detection.page_cropping import PageCroppingStepOutput  # noqa: E402
from vkit.pipeline.text_detection.page_text_region import PageTextRegionStepOutput  # noqa: E402
from vkit.utility import opt as ref_opt  # noqa: E402

OUT = os.path.join(HERE, 'text_region_cropping.npz')
LABELS = ('page_char_mask', 'page_char_height_score_map', 'page_char_gaussian_score_map', 'page_char_bounding_box_mask')
PLANES = ('page_image',) + LABELS


# ---- the stand-ins for shapely: closed boxes, brute force ----
class BoxPolygon:
    def __init__(self, minx, miny, maxx, maxy):
        self.minx, self.miny, self.maxx, self.maxy = minx, miny, maxx, maxy


class PointGeometry:
    def __init__(self, x, y):
        self.x, self.y = x, y


class BruteForceTree:
    def __init__(self, points):
        self.points = list(points)

    def query(self, polygon, predicate=None):
        assert predicate == 'intersects'
        hits = [k for k, p in enumerate(self.points)
                if polygon.minx <= p.x <= polygon.maxx and polygon.miny <= p.y <= polygon.maxy]
        return hits[::-1]


def make_page(rng, shape):
    image = np.stack([blocky(rng, shape, 4, 0, 16, np.uint8) * np.uint8(17) for _ in range(3)], axis=2)
    return dict(page_image=image, page_char_mask=boxes_mask(rng, shape, 60, 6),
                page_char_height_score_map=blocky(rng, shape, 4, 0, 8, np.float32) * np.float32(1.37),
                page_char_gaussian_score_map=blocky(rng, shape, 4, 0, 5, np.float32) / np.float32(4),
                page_char_bounding_box_mask=boxes_mask(rng, shape, 40, 9))


def char_quad(rng, cy, cx):
    """a convex quad around (cy, cx): (4, 2) (y, x), up-left, up-right, down-right, down-left"""
    hh, hw = rng.uniform(3, 6), rng.uniform(3, 6)
    q = np.array([(-hh, -hw), (-hh, hw), (hh, hw), (hh, -hw)]) + rng.uniform(-0.7, 0.7, (4, 2))
    return np.round(q + (cy, cx), 3)


def make_chars(rng, shape, n_chars):
    """-> rows (tag, char_idx, smooth y, smooth x, quad): a centroid label and 0 .. 2 deviate labels a char"""
    rows = []
    for g in range(n_chars):
        q = char_quad(rng, rng.uniform(0, shape[0]), rng.uniform(0, shape[1]))
        cy, cx = np.round(q.mean(axis=0), 3).tolist()
        rows.append((0, g, cy, cx, q))
        for _ in range(int(rng.integers(0, 3))):
            w = rng.dirichlet(np.ones(4) * 3)
            dy, dx = np.round((q * w[:, None]).sum(axis=0), 3).tolist()
            rows.append((1, g, dy, dx, q))
    return rows


def edge_chars(core, first):
    """chars around the first window's core box (up, down, left, right): centroid labels exactly on each edge and corner (their
    deviate labels one pixel outside), and centroid labels one pixel outside whose deviate labels lie on the edge"""
    up, down, left, right = core
    my, mx = (up + down) // 2, (left + right) // 2
    on_edge = [(up, mx), (down, mx), (my, left), (my, right), (up, left), (up, right), (down, left), (down, right)]
    outward = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]
    rows = []
    g = first
    for (y, x), (oy, ox) in zip(on_edge, outward):
        sy, sx = (0, 3) if ox == 0 else (3, 0)        # the second char slides along the edge
        for cen, dev in (((y, x), (y + oy, x + ox)), ((y + sy + oy, x + sx + ox), (y + sy, x + sx))):
            if (y, x) in on_edge[4:] and cen != (y, x):
                continue
            q = np.array([(-5, -5), (-5, 5), (5, 5), (5, -5)], np.float64) + cen
            rows.append((0, g, float(cen[0]), float(cen[1]), q))
            rows.append((1, g, float(dev[0]), float(dev[1]), q))
            g += 1
    return rows


def ref_labels(rows):
    tags = (L.PageCharRegressionLabelTag.CENTROID, L.PageCharRegressionLabelTag.DEVIATE)
    out = []
    for tag, g, y, x, q in rows:
        corners = [Point.create(y=float(py), x=float(px)) for py, px in q.tolist()]
        out.append(L.PageCharRegressionLabel(char_idx=g, tag=tags[tag], label_point_smooth_y=y, label_point_smooth_x=x,
                                             downsampled_label_point_y=round(y), downsampled_label_point_x=round(x),
                                             up_left=corners[0], up_right=corners[1], down_right=corners[2],
                                             down_left=corners[3]))
        assert out[-1].valid
    return out


BASE = dict(core_size=32, pad_size=8, num_centroid_points_min=3, num_deviate_points_min=2)
# (name, shape before the rotation, angle, config overrides, chars, cropped pages); each run with three seeds
CASES = [
    ('plain', (96, 128), 0, dict(BASE), 200, 3),
    ('rotate90', (80, 110), 90, dict(BASE), 200, 3),
    ('rotate37', (80, 100), 37, dict(BASE, num_centroid_points_min=2, num_deviate_points_min=1), 200, 3),
    ('rotate200', (70, 90), 200, dict(BASE), 150, 2),
    ('short_axis', (24, 160), 0, dict(BASE, num_centroid_points_min=2, num_deviate_points_min=1), 80, 3),
    ('both_axes', (24, 28), 0, dict(BASE, num_centroid_points_min=2, num_deviate_points_min=1), 40, 2),
    ('pad_value', (60, 70), 0, dict(BASE, pad_value=77), 120, 2),
    ('factor4', (80, 80), 0, dict(BASE, downsample_labeling_factor=4), 150, 2),
    ('no_downsample', (80, 80), 0, dict(BASE, enable_downsample_labeling=False), 150, 2),
    ('default_thresholds', (64, 64), 0, dict(core_size=32, pad_size=8), 400, 2),
    ('rejects_all', (96, 96), 0, dict(BASE, num_centroid_points_min=10000), 100, 2),
    ('rejects_most', (128, 128), 0, dict(BASE, num_centroid_points_min=11, num_deviate_points_min=9), 120, 3),
    ('factor_half', (96, 96), 0, dict(BASE, num_samples_factor_relative_to_num_cropped_pages=0.5), 180, 3),
    ('factor_two', (96, 96), 0, dict(BASE, num_samples_factor_relative_to_num_cropped_pages=2.0), 180, 2),
    ('edges', (96, 112), 0, dict(BASE), 60, 1),
]
SEEDS = (0, 1, 2)


def box4(b):
    return [int(b.up), int(b.down), int(b.left), int(b.right)]


def main():
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    TC.STRtree, TC.ShapelyPoint = BruteForceTree, PointGeometry
    ref_box.build_shapely_polygon_as_box = BoxPolygon
    ref_opt._cattrs.structure = lambda mapping, cls: cls(**mapping)
    croppers = []
    saved_init = ref_cropper.Cropper.__init__

    def recording_init(self, cropper_state):
        saved_init(self, cropper_state)
        croppers.append(cropper_state)

    ref_cropper.Cropper.__init__ = recording_init
    packed, index, pages = {}, [], []

    def put(array):
        """Append ``array`` to the flat array of its dtype: -> [offset, shape, dtype] for the index."""
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    for k, (name, shape_before, angle, overrides, n_chars, n_pages) in enumerate(CASES):
        shape = tuple(rotate.distort({'angle': angle}, shapable_or_shape=shape_before).shape) if angle else shape_before
        planes = make_page(default_rng(20_000 + k), shape)
        pages.append({n: put(planes[n]) for n in PLANES})
        for seed in SEEDS:
            config = TC.PageTextRegionCroppingStepConfig(**overrides)
            rows = make_chars(default_rng(30_000 + 10 * k + seed), shape, n_chars)
            if name == 'edges':
                first = ref_cropper.Cropper.create_from_random_proposal(shape=shape, core_size=config.core_size,
                                                                        pad_size=config.pad_size, rng=default_rng(seed))
                rows += edge_chars(box4(first.original_core_box), n_chars)
            keys = [(t, g, y, x) for t, g, y, x, _ in rows]
            assert len(set(keys)) == len(keys)
            labels = ref_labels(rows)
            by_tag = [[lb for lb, r in zip(labels, rows) if r[0] == tag] for tag in (0, 1)]
            step_input = TC.PageTextRegionCroppingStepInput(
                page_cropping_step_output=PageCroppingStepOutput(cropped_pages=[None] * n_pages),
                page_text_region_step_output=PageTextRegionStepOutput(
                    page_image=Image(mat=planes['page_image']), page_active_mask=Mask(mat=np.ones(shape, np.uint8)),
                    page_char_polygons=[], page_text_region_polygons=[], page_char_polygon_text_region_polygon_indices=[],
                    shape_before_rotate=shape_before, rotate_angle=angle, debug=None),
                page_text_region_label_step_output=L.PageTextRegionLabelStepOutput(
                    page_char_mask=Mask(mat=planes['page_char_mask']),
                    page_char_height_score_map=ScoreMap(mat=planes['page_char_height_score_map'], is_prob=False),
                    page_char_gaussian_score_map=ScoreMap(mat=planes['page_char_gaussian_score_map']),
                    page_char_regression_labels=labels,
                    page_char_bounding_box_mask=Mask(mat=planes['page_char_bounding_box_mask'])))
            rng = default_rng(seed)
            del croppers[:]
            got = TC.PageTextRegionCroppingStep(config).run(step_input, rng)
            state = rng.bit_generator.state['state']
            row = dict(name=name, seed=seed, page=k, shape=list(shape), shape_before_rotate=list(shape_before), angle=angle,
                       config=overrides, num_cropped_pages=n_pages, rng_state=[str(state['state']), str(state['inc'])],
                       label_key=put(np.array([(t, g) for t, g, *_ in rows], np.int64).reshape(-1, 2)),
                       label_smooth=put(np.array([(y, x) for _, _, y, x, _ in rows], np.float64).reshape(-1, 2)),
                       label_quad=put(np.array([q for *_, q in rows], np.float64).reshape(-1, 4, 2)),
                       croppers=[box4(s.original_box) + box4(s.target_box) + box4(s.original_core_box) for s in croppers],
                       samples=[])
            # the croppers of the samples: with a rotation every attempt makes two, the window is the second
            per_attempt = 2 if angle else 1
            windows = croppers[per_attempt - 1::per_attempt]
            cursor = 0
            for sample in got.cropped_page_text_regions:
                out = sample.page_char_regression_labels
                # the window of this sample: the next attempt whose offsets reproduce the sample's labels
                found = None
                while found is None:
                    s = windows[cursor]
                    cursor += 1
                    oy, ox = s.target_box.up - s.original_box.up, s.target_box.left - s.original_box.left
                    want = [(lb.tag, lb.char_idx, lb.label_point_smooth_y, lb.label_point_smooth_x) for lb in out]
                    # the output is a subsequence of the centroid labels followed by one of the deviate labels
                    kept, at = ([], []), 0
                    for tag, group in enumerate(by_tag):
                        for i, lb in enumerate(group):
                            if at < len(want) and want[at] == (lb.tag, lb.char_idx, lb.label_point_smooth_y + oy,
                                                               lb.label_point_smooth_x + ox):
                                kept[tag].append(i)
                                at += 1
                    if at == len(want) and box4(s.target_core_box) == box4(sample.target_core_box):
                        found = (cursor - 1, kept[0], kept[1])
                attempt, kept_c, kept_d = found
                rec = dict(attempt=attempt, target_core_box=box4(sample.target_core_box),
                           kept_centroid=put(np.array(kept_c, np.int64)), kept_deviate=put(np.array(kept_d, np.int64)),
                           shifted=put(np.array([(lb.label_point_smooth_y, lb.label_point_smooth_x, lb.downsampled_label_point_y,
                                                  lb.downsampled_label_point_x, lb.up_left.smooth_y, lb.up_left.smooth_x,
                                                  lb.down_right.smooth_y, lb.down_right.smooth_x) for lb in out],
                                                np.float64).reshape(-1, 8)),
                           planes={'page_image': put(sample.page_image.mat)})
                for n in LABELS:
                    element = getattr(sample, n)
                    assert element.box == sample.target_core_box
                    rec['planes'][n] = put(element.mat)
                d = sample.downsampled_label
                if d is not None:
                    rec['down_shape'] = [int(v) for v in d.shape]
                    rec['down_target_core_box'] = box4(d.target_core_box)
                    rec['down_points'] = put(np.array([(lb.downsampled_label_point_y, lb.downsampled_label_point_x,
                                                        int(lb.is_downsampled), lb.downsample_labeling_factor)
                                                       for lb in d.page_char_regression_labels], np.int64).reshape(-1, 4))
                    for n in LABELS:
                        rec['planes']['down_' + n] = put(getattr(d, n).mat)
                row['samples'].append(rec)
            index.append(row)

    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(dict(pages=pages, runs=index)))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')
    for row in index:
        print(row['name'], row['seed'], 'labels', row['label_key'][1][0], 'croppers', len(row['croppers']), 'samples',
              [(s['attempt'], s['kept_centroid'][1][0], s['kept_deviate'][1][0]) for s in row['samples']])


if __name__ == '__main__':
    main()
