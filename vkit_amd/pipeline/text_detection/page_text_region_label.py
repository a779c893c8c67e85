"""PageTextRegionLabelStep: the text-region training labels of a page (reference:
vkit/pipeline/text_detection/page_text_region_label.py).

The step runs the reference's five parts in its order, with its exceptions:
  1. the char mask and the char-height score map: ONE ordered polygon paint (csrc/polygon.hip) of the chars sorted by
     ``reversed(argsort(rectangular heights))`` -- the last writer wins, so the smallest height survives where chars overlap;
     the default char-mask engine ignores the bounding polygons and leaves ``char_masks`` None, so the height map takes the
     polygon branch, and a tie in the sort writes equal values;
  2. the Gaussian char score map: the default char-heatmap engine (csrc/char_heatmap.hip);
  3. the char regression labels: the centres, the generator draws (one ``rng.integers`` over the interleaved bounds, which
     equals the reference's two scalar draws per candidate) and every check the host can make are vectorised here; ONE launch
     of vkx_region_label_deviate_dev (csrc/region_label.hip) maps every candidate, reports its status and classifies it against
     every centre, then the step's only synchronisation brings the records back.  A candidate whose own centre ties with
     another at the minimum distance is resolved by sklearn's KDTree, as the reference resolves it;
  4. the char bounding-box mask and the inactive region: ONE launch of vkx_region_label_planes_dev.  Every label of a char
     shares its corners and every char has a centroid label, so the mask is the union of the chars' floor / ceil boxes and
     does not wait for step 3; the exception the reference's Box.fill_mask raises is decided before the launch.
A device-resident page keeps its planes on the device; a host page gives host planes."""
import logging
import math
from enum import Enum, unique
from typing import Any, List, Mapping, Optional, Sequence

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Mask, Point, ScoreMap
from vkit_amd.element.polygon import polygon_centroids
from vkit_amd.engine.char_heatmap import (
    CharHeatmapDefaultEngineInitConfig,
    char_heatmap_default_engine_executor_factory,
)
from vkit_amd.engine.char_mask.external_ellipse import char_quads
from vkit_amd.utility import normalize_to_probs
from ..interface import PipelineStep, PipelineStepFactory
from .page_distortion import paint_polygons
from .page_text_region import PageTextRegionStepOutput

logger = logging.getLogger(__name__)

_MAX_SIDE = 32768


def _lazy():
    return attrs.field(default=None, init=False, repr=False)


def _unwrap(value):
    assert value is not None
    return value


@attrs.define
class PageTextRegionLabelStepConfig:
    char_heatmap_default_engine_init_config: CharHeatmapDefaultEngineInitConfig = \
        attrs.field(factory=CharHeatmapDefaultEngineInitConfig)
    char_mask_engine_config: Mapping[str, Any] = attrs.field(factory=lambda: {'type': 'default'})

    # The centroid label and up to this many deviate labels per char.
    num_deviate_char_regression_labels: int = 1
    num_deviate_char_regression_labels_candiates_factor: int = 3


@attrs.define
class PageTextRegionLabelStepInput:
    page_text_region_step_output: PageTextRegionStepOutput


@unique
class PageCharRegressionLabelTag(Enum):
    CENTROID = 'centroid'
    DEVIATE = 'deviate'


PI = float(np.pi)
TWO_PI = float(2 * np.pi)


@attrs.define
class Vector:
    y: float
    x: float

    _distance: Optional[float] = _lazy()
    _theta: Optional[float] = _lazy()

    def lazy_post_init(self):
        if self._distance is None:
            self._distance = math.hypot(self.x, self.y)
            self._theta = float(np.arctan2(self.y, self.x)) % TWO_PI

    @property
    def distance(self):
        self.lazy_post_init()
        return _unwrap(self._distance)

    @property
    def theta(self):
        self.lazy_post_init()
        return _unwrap(self._theta)

    @classmethod
    def calculate_theta_delta(cls, vector0: 'Vector', vector1: 'Vector', clockwise: bool = False):
        delta = (vector1.theta - vector0.theta + PI) % TWO_PI - PI
        if clockwise and delta < 0:
            delta += TWO_PI
        return delta

    def dot(self, other: 'Vector'):
        return self.x * other.x + self.y * other.y


@attrs.define
class PageCharRegressionLabel:
    char_idx: int
    tag: PageCharRegressionLabelTag
    label_point_smooth_y: float
    label_point_smooth_x: float
    downsampled_label_point_y: int
    downsampled_label_point_x: int
    up_left: Point
    up_right: Point
    down_right: Point
    down_left: Point

    is_downsampled: bool = False
    downsample_labeling_factor: int = 1

    # bounding fields: from the corners alone
    _bounding_smooth_up: Optional[float] = _lazy()
    _bounding_smooth_down: Optional[float] = _lazy()
    _bounding_smooth_left: Optional[float] = _lazy()
    _bounding_smooth_right: Optional[float] = _lazy()
    _bounding_orientation_idx: Optional[int] = _lazy()

    # the rest: from the corners relative to the label point
    _up_left_vector: Optional[Vector] = _lazy()
    _up_right_vector: Optional[Vector] = _lazy()
    _down_right_vector: Optional[Vector] = _lazy()
    _down_left_vector: Optional[Vector] = _lazy()

    _up_left_to_up_right_angle: Optional[float] = _lazy()
    _up_right_to_down_right_angle: Optional[float] = _lazy()
    _down_right_to_down_left_angle: Optional[float] = _lazy()
    _down_left_to_up_left_angle: Optional[float] = _lazy()
    _valid: Optional[bool] = _lazy()
    _clockwise_angle_distribution: Optional[Sequence[float]] = _lazy()

    @property
    def corner_points(self):
        yield from (self.up_left, self.up_right, self.down_right, self.down_left)

    @classmethod
    def get_bounding_orientation_idx(cls, down_left: Point, down_right: Point):
        """The side of the bounding box the char's bottom edge faces: 0 up, 1 down, 2 left, 3 right, from the angle of the
        down-left -> down-right vector."""
        factor = Vector(y=down_right.smooth_y - down_left.smooth_y, x=down_right.smooth_x - down_left.smooth_x).theta / PI
        if 1.75 <= factor or factor < 0.25:
            return 1
        if 0.25 <= factor < 0.75:
            return 2
        if 0.75 <= factor < 1.25:
            return 0
        if 1.25 <= factor:
            return 3
        raise RuntimeError()

    def lazy_post_init(self):
        if self._bounding_smooth_up is None:
            ys = [point.smooth_y for point in self.corner_points]
            xs = [point.smooth_x for point in self.corner_points]
            self._bounding_smooth_up, self._bounding_smooth_down = min(ys), max(ys)
            self._bounding_smooth_left, self._bounding_smooth_right = min(xs), max(xs)
            self._bounding_orientation_idx = self.get_bounding_orientation_idx(down_left=self.down_left,
                                                                               down_right=self.down_right)
        if self._up_left_vector is not None:
            return

        vectors = [
            Vector(y=point.smooth_y - self.label_point_smooth_y, x=point.smooth_x - self.label_point_smooth_x)
            for point in self.corner_points
        ]
        self._up_left_vector, self._up_right_vector, self._down_right_vector, self._down_left_vector = vectors
        angles = [Vector.calculate_theta_delta(vectors[k], vectors[(k + 1) % 4], clockwise=True) for k in range(4)]
        (self._up_left_to_up_right_angle, self._up_right_to_down_right_angle, self._down_right_to_down_left_angle,
         self._down_left_to_up_left_angle) = angles
        # valid when the clockwise angles around the label point add up to a full turn (within about 4 degrees)
        self._valid = math.isclose(sum(angles), TWO_PI, rel_tol=0.012)
        self._clockwise_angle_distribution = normalize_to_probs(angles)

    def copy(self, with_non_bounding_related_lazy_fields: bool = False):
        copied = attrs.evolve(self)
        if with_non_bounding_related_lazy_fields:
            # the bounding fields are left to be computed again
            for name in ('_up_left_vector', '_up_right_vector', '_down_right_vector', '_down_left_vector',
                         '_up_left_to_up_right_angle', '_up_right_to_down_right_angle', '_down_right_to_down_left_angle',
                         '_down_left_to_up_left_angle', '_valid', '_clockwise_angle_distribution'):
                setattr(copied, name, getattr(self, name))
        return copied

    def to_shifted_page_char_regression_label(self, offset_y: int, offset_x: int):
        assert self.valid and not self.is_downsampled
        # a shift leaves the label point relative to the corners as it was
        shifted = self.copy(with_non_bounding_related_lazy_fields=True)
        shifted.label_point_smooth_y = self.label_point_smooth_y + offset_y
        shifted.label_point_smooth_x = self.label_point_smooth_x + offset_x
        shifted.downsampled_label_point_y = int(shifted.label_point_smooth_y)
        shifted.downsampled_label_point_x = int(shifted.label_point_smooth_x)
        shifted.up_left = self.up_left.to_shifted_point(offset_y=offset_y, offset_x=offset_x)
        shifted.up_right = self.up_right.to_shifted_point(offset_y=offset_y, offset_x=offset_x)
        shifted.down_right = self.down_right.to_shifted_point(offset_y=offset_y, offset_x=offset_x)
        shifted.down_left = self.down_left.to_shifted_point(offset_y=offset_y, offset_x=offset_x)
        return shifted

    def to_downsampled_page_char_regression_label(self, downsample_labeling_factor: int):
        assert self.valid and not self.is_downsampled
        downsampled = self.copy(with_non_bounding_related_lazy_fields=True)
        # a downsampled label takes no further shift or downsampling
        downsampled.is_downsampled = True
        downsampled.downsample_labeling_factor = downsample_labeling_factor
        downsampled.downsampled_label_point_y = int(self.label_point_smooth_y // downsample_labeling_factor)
        downsampled.downsampled_label_point_x = int(self.label_point_smooth_x // downsample_labeling_factor)
        return downsampled

    @property
    def bounding_smooth_up(self):
        self.lazy_post_init()
        return _unwrap(self._bounding_smooth_up)

    @property
    def bounding_smooth_down(self):
        self.lazy_post_init()
        return _unwrap(self._bounding_smooth_down)

    @property
    def bounding_smooth_left(self):
        self.lazy_post_init()
        return _unwrap(self._bounding_smooth_left)

    @property
    def bounding_smooth_right(self):
        self.lazy_post_init()
        return _unwrap(self._bounding_smooth_right)

    @property
    def bounding_center_point(self):
        return Point.create(y=(self.bounding_smooth_up + self.bounding_smooth_down) / 2,
                            x=(self.bounding_smooth_left + self.bounding_smooth_right) / 2)

    @property
    def bounding_smooth_shape(self):
        return (self.bounding_smooth_down - self.bounding_smooth_up, self.bounding_smooth_right - self.bounding_smooth_left)

    @property
    def bounding_orientation_idx(self):
        self.lazy_post_init()
        return _unwrap(self._bounding_orientation_idx)

    @property
    def valid(self):
        self.lazy_post_init()
        return _unwrap(self._valid)

    def generate_up_left_offsets(self):
        self.lazy_post_init()
        vector = _unwrap(self._up_left_vector)
        return vector.y, vector.x

    def generate_clockwise_angle_distribution(self):
        self.lazy_post_init()
        return _unwrap(self._clockwise_angle_distribution)

    def generate_clockwise_distances(self):
        self.lazy_post_init()
        return tuple(_unwrap(v).distance for v in (self._up_left_vector, self._up_right_vector, self._down_right_vector,
                                                   self._down_left_vector))


@attrs.define
class PageTextRegionLabelStepOutput:
    page_char_mask: Mask
    page_char_height_score_map: ScoreMap
    page_char_gaussian_score_map: ScoreMap
    page_char_regression_labels: Sequence[PageCharRegressionLabel]
    page_char_bounding_box_mask: Mask


def labels_valid(label_y: np.ndarray, label_x: np.ndarray, quads: np.ndarray) -> np.ndarray:
    """PageCharRegressionLabel.valid of many labels at once: label points float64 (K,), their chars' corners float64 (K, 4, 2)
    (x, y) in the order up-left, up-right, down-right, down-left.  The reference's scalar expressions, elementwise:
    theta = arctan2(dy, dx) % 2 pi, the clockwise deltas, their sum from the left, and math.isclose(sum, 2 pi, rel_tol=0.012)
    (tests/test_text_region_label_golden.py compares both forms)."""
    vy = quads[:, :, 1] - label_y[:, None]
    vx = quads[:, :, 0] - label_x[:, None]
    theta = np.remainder(np.arctan2(vy, vx), TWO_PI)
    total = np.zeros(len(label_y))
    for k in range(4):
        delta = np.remainder(theta[:, (k + 1) % 4] - theta[:, k] + PI, TWO_PI) - PI
        delta = np.where(delta < 0, delta + TWO_PI, delta)
        total = total + delta
    diff = np.abs(TWO_PI - total)
    return (total == TWO_PI) | (diff <= abs(0.012 * TWO_PI)) | (diff <= np.abs(0.012 * total))


def draw_highs(boxes_hw: np.ndarray, m: int) -> np.ndarray:
    """The bounds of the reference's draws, interleaved in its order: per char, m times (bh - 1, bw - 1)."""
    return np.repeat((boxes_hw - 1).astype(np.int64), m, axis=0).reshape(-1)


def box_fill_plan(up, down, left, right, shape):
    """Box(up, down, left, right).fill_mask(page mask) of the reference, decided from the box: (exception or None, the
    region it writes as (up, down, left, right) inside the page, or None when it writes nothing).  A box of the page's shape
    is not extracted and fills the whole page; any other box must satisfy 0 <= up <= down <= h (and so for x), and fills its
    part inside the page."""
    h, w = shape
    if (down - up + 1, right - left + 1) == (h, w):
        return None, (0, h - 1, 0, w - 1)
    if not (0 <= up <= down <= h and 0 <= left <= right <= w):
        return AssertionError(), None
    if up >= h or left >= w:
        return None, None
    return None, (up, min(down, h - 1), left, min(right, w - 1))


def _resolve_ties(centres: np.ndarray, points: np.ndarray, owners: np.ndarray) -> np.ndarray:
    """Keep flags of the tied candidates: KDTree(centres).query(points) returns the owner, as the reference's tree does; without
    sklearn, the lowest index at the minimum distance."""
    try:
        from sklearn.neighbors import KDTree
    except ImportError:
        logger.warning('sklearn is not importable: tied deviate candidates go to the lowest centre index')
        keep = np.empty(len(points), bool)
        c = centres.astype(np.int64)
        for k, (p, owner) in enumerate(zip(points.astype(np.int64), owners)):
            d = ((c - p) ** 2).sum(axis=1)
            keep[k] = int(np.flatnonzero(d == d.min())[0]) == owner
        return keep
    _, nearest = KDTree(centres).query(points)
    return nearest[:, 0] == owners


class PageTextRegionLabelStep(PipelineStep[PageTextRegionLabelStepConfig, PageTextRegionLabelStepInput,
                                           PageTextRegionLabelStepOutput]):

    def __init__(self, config: PageTextRegionLabelStepConfig):
        super().__init__(config)
        self.char_heatmap_default_engine_executor = char_heatmap_default_engine_executor_factory.create(
            config.char_heatmap_default_engine_init_config)
        engine_type = (config.char_mask_engine_config or {}).get('type')
        if engine_type == 'external_ellipse':
            raise NotImplementedError('the external_ellipse char-mask engine does not take char_bounding_polygons, which '
                                      'this step always passes')
        if engine_type != 'default':
            raise NotImplementedError(f'char mask engine "{engine_type}" is outside the accelerated path')
        for name in ('num_deviate_char_regression_labels', 'num_deviate_char_regression_labels_candiates_factor'):
            value = getattr(config, name)
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise TypeError(f'{name} must be an int')

    def _regression(self, shape, polygons, quads, rng: RandomGenerator, ctx):
        """generate_page_char_regression_labels: -> (labels, exception or None).  The generator ends where the reference's
        ends, the exception included."""
        config = self.config
        n = len(quads)
        if n == 0:
            # KDTree of no centres: sklearn's check_array refuses the empty array
            return [], ValueError('no char to build the centre tree from')
        centres_smooth = polygon_centroids(quads)
        if not np.isfinite(centres_smooth).all():
            return [], ValueError('non-finite char centroid')
        centres = np.rint(centres_smooth)
        if (np.abs(centres) >= 2**30).any():
            return [], ValueError('char centroid outside +-2^30')
        centres = centres.astype(np.int32)                                # (x, y), PointList.to_np_array
        centroid_valid = labels_valid(centres_smooth[:, 1], centres_smooth[:, 0], quads)

        num = int(config.num_deviate_char_regression_labels)
        m = int(config.num_deviate_char_regression_labels_candiates_factor) * num
        points = np.rint(quads)
        box_ul = np.stack([points[:, :, 1].min(axis=1), points[:, :, 0].min(axis=1)], axis=1).astype(np.int64)
        box_hw = np.stack([points[:, :, 1].max(axis=1), points[:, :, 0].max(axis=1)], axis=1).astype(np.int64) - box_ul + 1

        # the first char the host alone sees fail, and how: its centroid label is not valid (AssertionError), or its draws
        # cannot be made (ValueError: no candidates at all with num > 0, or a box side below 3)
        fails = ~centroid_valid
        if num > 0:
            fails |= (m <= 0) | (box_hw[:, 0] < 3) | (box_hw[:, 1] < 3)
        k_host = int(np.argmax(fails)) if fails.any() else n
        k_lim = k_host if num > 0 else 0
        highs = draw_highs(box_hw[:k_lim], max(m, 0))
        state = rng.bit_generator.state
        draws = rng.integers(1, highs) if highs.size else np.zeros(0, np.int64)

        records = None
        k_dev = n
        if k_lim > 0 and m > 0:
            draws_xy = draws.reshape(k_lim, m, 2)[:, :, ::-1]
            records = _native.region_label_deviate(quads[:k_lim], centres, draws_xy, shape, ctx=ctx)
            status = records['status']
            bad = ((status == 3) | (status == 2)).any(axis=1)
            if bad.any():
                k_dev = int(np.argmax(bad))
        k_exc = min(k_host, k_dev)

        # the labels of the chars before the failing one (their warnings are emitted before the exception)
        selected = np.zeros((k_exc, max(m, 0)), bool)
        if records is not None and k_exc > 0:
            rec = records[:k_exc]
            keep = (rec['status'] == 0) & (rec['cls'] == 0)
            tied = (rec['status'] == 0) & (rec['cls'] == 2)
            if tied.any():
                owners = np.nonzero(tied)[0]
                tied_points = np.stack([rec['ix'][tied], rec['iy'][tied]], axis=1).astype(np.int32)
                keep[tied] = _resolve_ties(centres, tied_points, owners)
            if keep.any():
                valid = np.zeros_like(keep)
                char_of = np.nonzero(keep)[0]
                valid[keep] = labels_valid(rec['y'][keep], rec['x'][keep], quads[char_of])
                keep &= valid
            selected = keep & (np.cumsum(keep, axis=1) <= num)
        labels: List[PageCharRegressionLabel] = []
        for g in range(k_exc):
            up_left, up_right, down_right, down_left = polygons[g].points
            cx, cy = centres_smooth[g].tolist()
            labels.append(PageCharRegressionLabel(
                char_idx=g, tag=PageCharRegressionLabelTag.CENTROID, label_point_smooth_y=cy, label_point_smooth_x=cx,
                downsampled_label_point_y=int(centres[g, 1]), downsampled_label_point_x=int(centres[g, 0]),
                up_left=up_left, up_right=up_right, down_right=down_right, down_left=down_left))
            if num <= 0:
                continue
            count = 0
            for j in np.flatnonzero(selected[g]).tolist():
                r = records[g, j]
                labels.append(PageCharRegressionLabel(
                    char_idx=g, tag=PageCharRegressionLabelTag.DEVIATE, label_point_smooth_y=float(r['y']),
                    label_point_smooth_x=float(r['x']), downsampled_label_point_y=int(r['iy']),
                    downsampled_label_point_x=int(r['ix']), up_left=up_left, up_right=up_right, down_right=down_right,
                    down_left=down_left))
                count += 1
            if count < num:
                logger.warning(f'Cannot sample enough deviate labels for char_polygon={polygons[g]}')

        if k_exc == n:
            return labels, None
        if k_dev < k_host:
            # every draw of the failing char was made before its points were mapped
            rng.bit_generator.state = state
            rng.integers(1, draw_highs(box_hw[:k_dev + 1], m))
            return labels, (ValueError('non-finite deviate point') if (records['status'][k_dev] == 3).any()
                            else AssertionError())
        if not centroid_valid[k_host]:
            return labels, AssertionError()
        if m <= 0:
            return labels, ValueError('no deviate candidates to map')
        # the reference's own draw raises: rng.integers(1, bh - 1), then rng.integers(1, bw - 1)
        bh, bw = box_hw[k_host].tolist()
        try:
            rng.integers(1, bh - 1)
            rng.integers(1, bw - 1)
        except ValueError as e:
            return labels, e
        raise AssertionError('unreachable')

    def run(self, input: PageTextRegionLabelStepInput, rng: RandomGenerator):
        src = input.page_text_region_step_output
        page_active_mask = src.page_active_mask
        polygons = src.page_char_polygons
        shape = tuple(src.page_image.shape)
        on_device = src.page_image.on_device or page_active_mask.on_device
        if max(shape) > _MAX_SIDE:
            # the rounded points and their squared distances to the centres stay exact below this side
            raise ValueError('pages larger than 32768 on a side are refused')

        # 1. the char mask and the char-height score map
        quads = char_quads(polygons)
        heights = [(math.hypot(ul[1] - dl[1], ul[0] - dl[0]) + math.hypot(ur[1] - dr[1], ur[0] - dr[0])) / 2
                   for ul, ur, dr, dl in quads.tolist()]
        order = tuple(reversed(np.asarray(heights).argsort()))
        polygon_list = list(polygons)
        with _native.resident(True):
            char_mask, height_map = paint_polygons(shape, [polygon_list[k] for k in order],
                                                   values=[heights[k] for k in order], want_mask=True)
            # 2. the Gaussian char score map
            gaussian = self.char_heatmap_default_engine_executor.run(
                {'height': shape[0], 'width': shape[1], 'char_polygons': polygons}).score_map
        ctx = char_mask.arr.ctx

        # 4 (launched before 3 completes). the boxes of every char, and the exception the first bad one raises
        box_exception, regions = None, []
        for up, down, left, right in zip(np.floor(quads[:, :, 1].min(axis=1)).tolist(),
                                         np.ceil(quads[:, :, 1].max(axis=1)).tolist(),
                                         np.floor(quads[:, :, 0].min(axis=1)).tolist(),
                                         np.ceil(quads[:, :, 0].max(axis=1)).tolist()):
            exc, region = box_fill_plan(int(up), int(down), int(left), int(right), shape)
            if exc is not None:
                box_exception = exc
                break
            if region is not None:
                regions.append(region)
        box_mask = None
        if box_exception is None and len(quads):
            active = page_active_mask.arr
            if not isinstance(active, _native.DevArray):
                active = ctx.to_device(np.ascontiguousarray(active))
            elif active.ctx is not ctx:
                active.ctx.sync()
                active = _native.device_copy(active, ctx)
            box_mask = ctx.dev_empty(shape, np.uint8)
            _native.region_label_planes(np.asarray(regions, np.int32).reshape(-1, 4), active, char_mask.arr,
                                        height_map.arr, box_mask)

        # 3. the regression labels (the step's only synchronisation)
        labels, exception = self._regression(shape, polygon_list, quads, rng, ctx)
        if exception is not None:
            raise exception
        if box_exception is not None:
            raise box_exception

        def place(arr):
            return arr if on_device else arr.host()

        return PageTextRegionLabelStepOutput(
            page_char_mask=Mask(mat=place(char_mask.arr)),
            page_char_height_score_map=ScoreMap(mat=place(height_map.arr), is_prob=False),
            page_char_gaussian_score_map=gaussian if on_device else ScoreMap(mat=gaussian.arr.host()),
            page_char_regression_labels=labels,
            page_char_bounding_box_mask=Mask(mat=place(box_mask)),
        )


page_text_region_label_step_factory = PipelineStepFactory(PageTextRegionLabelStep)
