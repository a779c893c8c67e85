"""Polygon element (reference: vkit/element/polygon.py), reduced to what the distortion path touches:
vertex bookkeeping, integer bounding box, clipping / shifting / resizing of the vertex list, and the raster
``np_mask`` (``cv.fillPoly`` in the reference, polygon.py:70-77 -- here ``vkx_fill_poly_mask_u8`` on the GPU)
with the ``fill_*`` / ``extract_*`` operators built on it.  The per-cell rasterisation of the image-grid
distortions lives in the HIP grid kernels; shapely / pyclipper based operations are outside the accelerated path.
"""
import math
from typing import Iterable, Optional, Sequence, Tuple, Union

import attrs
import numpy as np

from .type import ElementSetOperationMode, Shapable


@attrs.define(frozen=True, eq=False)
class Polygon:
    # ``Polygon(points=...)`` as in the reference; a polygon that came out of an array operator (``from_smooth_xy``)
    # holds its vertices as one float64 array and builds the ``PointTuple`` on first access of ``.points``
    _points: Optional['PointTuple'] = attrs.field(default=None, alias='points')

    _bounding_box: Optional['Box'] = attrs.field(default=None, init=False, repr=False)
    _np_mask: Optional[np.ndarray] = attrs.field(default=None, init=False, repr=False)
    _mask: Optional['Mask'] = attrs.field(default=None, init=False, repr=False)
    _smooth_xy: Optional[np.ndarray] = attrs.field(default=None, init=False, repr=False)

    def __attrs_post_init__(self):
        assert self._points is None or self._points

    @classmethod
    def create(cls, points: Union['PointList', 'PointTuple', Iterable['Point']]):
        return cls(points=PointTuple(points))

    @classmethod
    def from_smooth_xy(cls, smooth_xy: np.ndarray):
        """A polygon over the float64 (n, 2) array of smooth (x, y) vertices (``Point.create(y=y, x=x)`` per row, lazily)."""
        smooth_xy = np.asarray(smooth_xy, dtype=np.float64).reshape(-1, 2)
        assert smooth_xy.shape[0] > 0
        polygon = cls(points=None)
        object.__setattr__(polygon, '_smooth_xy', smooth_xy)
        return polygon

    @property
    def points(self) -> 'PointTuple':
        if self._points is None:
            assert self._smooth_xy is not None
            object.__setattr__(self, '_points', PointTuple(Point.create(y=float(y), x=float(x)) for x, y in self._smooth_xy))
        return self._points

    @property
    def smooth_xy(self) -> np.ndarray:
        """float64 (n, 2) smooth (x, y) of the vertices (cached)."""
        if self._smooth_xy is None:
            arr = np.empty((len(self._points), 2), np.float64)
            for k, p in enumerate(self._points):
                arr[k, 0] = p.smooth_x
                arr[k, 1] = p.smooth_y
            object.__setattr__(self, '_smooth_xy', arr)
        return self._smooth_xy

    @property
    def num_points(self):
        return self._smooth_xy.shape[0] if self._points is None else len(self._points)

    @property
    def bounding_box(self):
        if self._bounding_box is None:
            xy = self.to_smooth_np_array()  # integer positions as float32 (PointTuple quirk)
            box = Box(up=round(float(xy[:, 1].min())), down=round(float(xy[:, 1].max())),
                      left=round(float(xy[:, 0].min())), right=round(float(xy[:, 0].max())))
            object.__setattr__(self, '_bounding_box', box)
        return self._bounding_box

    def to_bounding_box(self):
        return self.bounding_box

    @property
    def area(self):
        """shapely's Polygon(integer points).area (reference polygon.py:48-53): the absolute shoelace sum of the ring, exact in
        float64 on integer vertices."""
        xy = self.to_np_array().astype(np.float64)
        x, y = xy[:, 0] - xy[0, 0], xy[:, 1] - xy[0, 1]
        return abs(float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))) / 2

    @property
    def self_relative_polygon(self):
        # reference polygon.py:105-138,59-64: shift by the (integer valued) minima, rebuild through from_np_array
        xy = self.to_smooth_np_array()
        xy[:, 0] -= xy[:, 0].min()
        xy[:, 1] -= xy[:, 1].min()
        return Polygon.from_np_array(xy)

    @property
    def np_mask(self):
        """Boolean raster over the bounding box (reference polygon.py:70-77), rasterised on the GPU."""
        if self._np_mask is None:
            from vkit_amd import _native
            raster = _native.fill_poly_mask(self.bounding_box.shape, self.self_relative_polygon.to_np_array())
            object.__setattr__(self, '_np_mask', raster.astype(np.bool_))
        return self._np_mask

    @property
    def mask(self):
        if self._mask is None:
            mask = Mask(mat=self.np_mask.astype(np.uint8)).to_box_attached(self.bounding_box)
            object.__setattr__(self, '_mask', mask)
        return self._mask

    # ---- measures (reference polygon.py:218-260)
    def get_center_point(self):
        """The polygon centroid of shapely (GEOS), over the smooth vertices: see ``polygon_centroids``."""
        if self.num_points < 3:
            raise ValueError('a polygon centroid needs at least 3 points')
        x, y = polygon_centroids(self.smooth_xy[None])[0].tolist()
        return Point.create(y=y, x=x)

    def get_rectangular_height(self):
        # the mean of the left and right sides (vertices up-left, up-right, down-right, down-left); math.hypot, as the
        # reference computes it (np.hypot may differ in the last bit)
        assert self.num_points == 4
        (ulx, uly), (urx, ury), (drx, dry), (dlx, dly) = self.smooth_xy.tolist()
        return (math.hypot(uly - dly, ulx - dlx) + math.hypot(ury - dry, urx - drx)) / 2

    def get_rectangular_width(self):
        assert self.num_points == 4
        (ulx, uly), (urx, ury), (drx, dry), (dlx, dly) = self.smooth_xy.tolist()
        return (math.hypot(uly - ury, ulx - urx) + math.hypot(dly - dry, dlx - drx)) / 2

    # ---- fills / extraction through the raster (reference polygon.py:439-503)
    def fill_np_array(self, mat: np.ndarray, value, alpha=1.0, keep_max_value: bool = False,
                      keep_min_value: bool = False):
        self.mask.fill_np_array(mat=mat, value=value, alpha=alpha, keep_max_value=keep_max_value,
                                keep_min_value=keep_min_value)

    def extract_mask(self, mask: 'Mask'):
        return self.mask.extract_mask(mask)

    def fill_mask(self, mask: 'Mask', value=1, keep_max_value: bool = False, keep_min_value: bool = False):
        self.mask.fill_mask(mask=mask, value=value, keep_max_value=keep_max_value, keep_min_value=keep_min_value)

    def fill_score_map(self, score_map: 'ScoreMap', value, keep_max_value: bool = False,
                       keep_min_value: bool = False):
        self.mask.fill_score_map(score_map=score_map, value=value, keep_max_value=keep_max_value,
                                 keep_min_value=keep_min_value)

    def extract_score_map(self, score_map: 'ScoreMap'):
        return self.mask.extract_score_map(score_map)

    def extract_image(self, image: 'Image'):
        return self.mask.extract_image(image)

    def fill_image(self, image: 'Image', value, alpha=1.0):
        self.mask.fill_image(image=image, value=value, alpha=alpha)

    # ---- conversion
    @classmethod
    def from_xy_pairs(cls, xy_pairs):
        return cls(points=PointTuple.from_xy_pairs(xy_pairs))

    def to_xy_pairs(self):
        return self.points.to_xy_pairs()

    def to_smooth_xy_pairs(self):
        return self.points.to_smooth_xy_pairs()

    @classmethod
    def from_flatten_xy_pairs(cls, flatten_xy_pairs: Sequence):
        return cls(points=PointTuple.from_flatten_xy_pairs(flatten_xy_pairs))

    def to_flatten_xy_pairs(self):
        return self.points.to_flatten_xy_pairs()

    def to_smooth_flatten_xy_pairs(self):
        return self.points.to_smooth_flatten_xy_pairs()

    @classmethod
    def from_np_array(cls, np_points: np.ndarray):
        return cls(points=PointTuple.from_np_array(np_points))

    def to_np_array(self):
        if self._points is None:
            return np.rint(self._smooth_xy).astype(np.int32)
        return self.points.to_np_array()

    def to_smooth_np_array(self):
        if self._points is None:     # PointTuple quirk: the integer positions as float32
            return np.rint(self._smooth_xy).astype(np.float32)
        return self.points.to_smooth_np_array()

    # ---- operators
    def to_clipped_points(self, shapable_or_shape: Union[Shapable, Tuple[int, int]]):
        return self.points.to_clipped_points(shapable_or_shape)

    def to_clipped_polygon(self, shapable_or_shape: Union[Shapable, Tuple[int, int]]):
        return Polygon(points=self.to_clipped_points(shapable_or_shape))

    def to_shifted_points(self, offset_y: int = 0, offset_x: int = 0):
        return self.points.to_shifted_points(offset_y=offset_y, offset_x=offset_x)

    def to_relative_points(self, origin_y: int, origin_x: int):
        return self.points.to_relative_points(origin_y=origin_y, origin_x=origin_x)

    def to_shifted_polygon(self, offset_y: int = 0, offset_x: int = 0):
        return Polygon(points=self.to_shifted_points(offset_y=offset_y, offset_x=offset_x))

    def to_relative_polygon(self, origin_y: int, origin_x: int):
        return Polygon(points=self.to_relative_points(origin_y=origin_y, origin_x=origin_x))

    def to_conducted_resized_polygon(self, shapable_or_shape, resized_height: Optional[int] = None,
                                     resized_width: Optional[int] = None):
        return Polygon(points=self.points.to_conducted_resized_points(
            shapable_or_shape, resized_height=resized_height, resized_width=resized_width))

    # ---- the bounding rectangle along a given angle (reference polygon.py:305-434): host float64, line for line
    @classmethod
    def project_polygon_to_unit_vector(cls, np_points: np.ndarray, radian: float):
        np_vector = np.asarray([math.cos(radian), math.sin(radian)])

        np_projected: np.ndarray = np.dot(np_points, np_vector.reshape(2, 1)).flatten()
        scale_begin = float(np_projected.min())
        scale_end = float(np_projected.max())

        np_point_begin = np_vector * scale_begin
        np_point_end = np_vector * scale_end

        return np_point_begin, np_point_end

    @classmethod
    def calculate_lines_intersection_point(cls, np_point0: np.ndarray, radian0: float, np_point1: np.ndarray,
                                           radian1: float):
        x0, y0 = np_point0
        x1, y1 = np_point1

        slope0 = np.tan(radian0)
        slope1 = np.tan(radian1)

        # Within pi / 2 + k * pi plus or minus 0.1 degree.
        invalid_slope_abs = 572.9572133543033

        if abs(slope0) > invalid_slope_abs and abs(slope1) > invalid_slope_abs:
            raise RuntimeError('Lines are vertical.')

        if abs(slope0) > invalid_slope_abs:
            its_x = float(x0)
            its_y = float(y1 + slope1 * (x0 - x1))

        elif abs(slope1) > invalid_slope_abs:
            its_x = float(x1)
            its_y = float(y0 + slope0 * (x1 - x0))

        else:
            c0 = y0 - slope0 * x0
            c1 = y1 - slope1 * x1

            with np.errstate(divide='ignore', invalid='ignore'):
                its_x = (c1 - c0) / (slope0 - slope1)
            if its_x == np.inf:
                raise RuntimeError('Lines not intersected.')

            its_y = slope0 * its_x + c0

        return Point.create(y=float(its_y), x=float(its_x))

    def to_bounding_rectangular_polygon(self, shape: Tuple[int, int], angle: Optional[float] = None):
        if angle is None:
            raise NotImplementedError(
                'the minimum rotated rectangle (shapely) is outside the accelerated path: pass the angle')

        # Make sure in range [0, 180).
        angle = angle % 180

        main_radian = math.radians(angle)
        orthogonal_radian = math.radians(angle + 90)

        # Project points.
        np_smooth_points = self.to_smooth_np_array()
        np_main_point_begin, np_main_point_end = self.project_polygon_to_unit_vector(
            np_points=np_smooth_points, radian=main_radian)
        np_orthogonal_point_begin, np_orthogonal_point_end = self.project_polygon_to_unit_vector(
            np_points=np_smooth_points, radian=orthogonal_radian)

        # Build polygon: (main begin, orthogonal begin), (main begin, orthogonal end), (main end, orthogonal end),
        # (main end, orthogonal begin).
        polygon = Polygon.create(points=[
            self.calculate_lines_intersection_point(np_point0=np_main_point, radian0=orthogonal_radian,
                                                    np_point1=np_orthogonal_point, radian1=main_radian)
            for np_main_point, np_orthogonal_point in (
                (np_main_point_begin, np_orthogonal_point_begin),
                (np_main_point_begin, np_orthogonal_point_end),
                (np_main_point_end, np_orthogonal_point_end),
                (np_main_point_end, np_orthogonal_point_begin),
            )
        ])

        # NOTE: Could be out-of-bound.
        return polygon.to_clipped_polygon(shape)


def generate_fill_by_polygons_mask(shape, polygons, mode):
    if mode == ElementSetOperationMode.UNION:
        return None
    return Mask.from_polygons(shape, polygons, mode)


def polygon_centroids(xy: np.ndarray) -> np.ndarray:
    """float64 (N, 2) centroids (x, y) of N polygons of k >= 3 smooth vertices each, ``xy`` float64 (N, k, 2).

    The reference takes ``shapely.Polygon(smooth points).centroid``, i.e. GEOS's algorithm::Centroid.  Shapely is not a
    dependency here, so this restates it (like the cv2 members, it is unpinned by an installed copy):
    over the closed ring p[0..k], triangles fanned from p[0]: cg3 += a2 * (p0 + p[i] + p[i+1]) and areasum2 += a2, with
    a2 = (p[i].x - p0.x) * (p[i+1].y - p0.y) - (p[i+1].x - p0.x) * (p[i].y - p0.y), and the centroid cg3 / 3 / areasum2.
    GEOS signs every a2 by the ring's orientation; negating every term negates both sums exactly, so the quotient does not
    depend on it.  A ring of zero area takes GEOS's fallback: the length-weighted mid points of its non-zero segments
    (length sqrt(dx * dx + dy * dy)), or its first point when it has none."""
    xy = np.asarray(xy, dtype=np.float64)
    ring = np.concatenate([xy, xy[:, :1]], axis=1)
    p0x, p0y = ring[:, 0, 0], ring[:, 0, 1]
    cg3x = np.zeros(len(xy))
    cg3y = np.zeros(len(xy))
    area2 = np.zeros(len(xy))
    line_x = np.zeros(len(xy))
    line_y = np.zeros(len(xy))
    length = np.zeros(len(xy))
    for i in range(ring.shape[1] - 1):
        ax, ay = ring[:, i, 0], ring[:, i, 1]
        bx, by = ring[:, i + 1, 0], ring[:, i + 1, 1]
        a2 = (ax - p0x) * (by - p0y) - (bx - p0x) * (ay - p0y)
        cg3x = cg3x + a2 * (p0x + ax + bx)
        cg3y = cg3y + a2 * (p0y + ay + by)
        area2 = area2 + a2
        dx, dy = ax - bx, ay - by
        seg = np.sqrt(dx * dx + dy * dy)
        nz = seg != 0.0
        length = np.where(nz, length + seg, length)
        line_x = np.where(nz, line_x + seg * ((ax + bx) / 2), line_x)
        line_y = np.where(nz, line_y + seg * ((ay + by) / 2), line_y)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.stack([cg3x / 3 / area2, cg3y / 3 / area2], axis=1)
        line = np.stack([line_x / length, line_y / length], axis=1)
    flat = ~(np.abs(area2) > 0.0)
    out[flat] = np.where((length > 0.0)[flat, None], line[flat], ring[flat, 0])
    return out


from .point import Point, PointList, PointTuple  # noqa: E402
from .box import Box  # noqa: E402
from .mask import Mask  # noqa: E402
from .score_map import ScoreMap  # noqa: E402
from .image import Image  # noqa: E402
