"""Float32 score / probability plane (reference: vkit/element/score_map.py).

On the hot path a ScoreMap is (a) an element that grid / affine distortions remap with float32 bilinear
weights and (b) the per-pixel alpha of a text-line layer in the page composite.
"""
from typing import Callable, Iterable, Optional, Tuple, Union

import attrs
import numpy as np

from vkit_amd import _native
from ._writable import LazyMat, WritableContext
from .opt import _deferred_stack, generate_shape_and_resized_shape
from .type import ElementSetOperationMode, Shapable


@attrs.define
class ScoreMapSetItemConfig:
    value: Union['ScoreMap', np.ndarray, float] = 1.0
    keep_max_value: bool = False
    keep_min_value: bool = False


@attrs.define
class NpVec:
    """A 2-D vector of numpy values with the cross product as ``*`` (reference score_map.py:36-56)."""
    x: np.ndarray
    y: np.ndarray

    @classmethod
    def from_point(cls, point: 'Point'):
        return cls(x=np.asarray(point.smooth_x, dtype=np.float32), y=np.asarray(point.smooth_y, dtype=np.float32))

    def __add__(self, other: 'NpVec'):
        return NpVec(x=self.x + other.x, y=self.y + other.y)

    def __sub__(self, other: 'NpVec'):
        return NpVec(x=self.x - other.x, y=self.y - other.y)

    def __mul__(self, other: 'NpVec') -> np.ndarray:
        return self.x * other.y - self.y * other.x


def quad_u(np_uv: np.ndarray) -> np.ndarray:
    """The u plane of a (h, w, 2) array of (u, v): as ``func_np_uv_to_mat`` it is recognised by identity and keeps
    ``fill_by_quad_interpolation`` on the device."""
    return np_uv[:, :, 0]


def quad_v(np_uv: np.ndarray) -> np.ndarray:
    """The v plane; see ``quad_u``."""
    return np_uv[:, :, 1]


@attrs.define(frozen=True, eq=False)
class ScoreMap(LazyMat, Shapable):
    _mat: np.ndarray = attrs.field(alias='mat')
    box: Optional['Box'] = None
    is_prob: bool = True

    def __attrs_post_init__(self):
        if self._mat.ndim != 2:
            raise RuntimeError('ndim should == 2.')
        if self.box and self.shape != self.box.shape:
            raise RuntimeError('self.shape != box.shape.')
        if self._mat.dtype != np.float32:
            raise RuntimeError('mat.dtype != np.float32')
        if isinstance(self._mat, np.ndarray):
            self._mat.flags.writeable = False
        if self.is_prob and self._mat.size:
            if self.mat.min() < 0.0 or self.mat.max() > 1.0:
                raise RuntimeError('score not in range [0.0, 1.0]')

    @classmethod
    def from_shape(cls, shape: Tuple[int, int], value: float = 0.0, is_prob: bool = True):
        height, width = shape
        if is_prob:
            assert 0.0 <= value <= 1.0
        return cls(mat=np.full((height, width), fill_value=value, dtype=np.float32), is_prob=is_prob)

    @classmethod
    def from_unchecked_mat(cls, mat, box: Optional['Box'] = None):
        """A probability map whose values are taken as they are, as ``assign_mat`` takes them (reference score_map.py: no range
        check): for a device-resident map, which the check would download, and for one that may hold NaN."""
        score_map = cls(mat=mat, box=box, is_prob=False)
        object.__setattr__(score_map, 'is_prob', True)
        return score_map

    @classmethod
    def from_shapable(cls, shapable: Shapable, value: float = 0.0, is_prob: bool = True):
        return cls.from_shape(shapable.shape, value=value, is_prob=is_prob)

    @property
    def height(self):
        return self._mat.shape[0]

    @property
    def width(self):
        return self._mat.shape[1]

    @property
    def equivalent_box(self):
        return self.box or Box.from_shapable(self)

    @property
    def writable_context(self):
        return WritableContext(self)

    def copy(self):
        return attrs.evolve(self, mat=self.mat.copy())

    def assign_mat(self, mat: np.ndarray):
        with self.writable_context:
            object.__setattr__(self, '_mat', mat)

    # ---- fills of a list of elements (reference score_map.py:315-520): vkit_amd/element/_sets.py
    @classmethod
    def unpack_element_value_pairs(cls, is_prob: bool, element_value_pairs):
        elements, values = [], []
        for element, value in element_value_pairs:
            elements.append(element)
            if is_prob:
                if isinstance(value, ScoreMap):
                    assert (0.0 <= value.mat).all() and (value.mat <= 1.0).all()
                elif isinstance(value, np.ndarray):
                    assert (0.0 <= value).all() and (value <= 1.0).all()
                elif isinstance(value, float):
                    assert 0.0 <= value <= 1.0
                else:
                    raise NotImplementedError()
            values.append(value)
        return elements, values

    def _fill_by_pairs(self, kind, pairs, mode, keep_max_value, keep_min_value, skip_values_uniqueness_check):
        elements, values = self.unpack_element_value_pairs(self.is_prob, pairs)
        _sets.fill_by(self, kind, elements, values, None, mode, keep_max_value, keep_min_value, skip_values_uniqueness_check)

    def fill_by_box_value_pairs(self, box_value_pairs, mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                keep_max_value: bool = False, keep_min_value: bool = False,
                                skip_values_uniqueness_check: bool = False):
        self._fill_by_pairs(_sets.BOXES, box_value_pairs, mode, keep_max_value, keep_min_value, skip_values_uniqueness_check)

    def fill_by_boxes(self, boxes: Iterable['Box'], value: Union['ScoreMap', np.ndarray, float] = 1.0,
                      mode: ElementSetOperationMode = ElementSetOperationMode.UNION, keep_max_value: bool = False,
                      keep_min_value: bool = False):
        self.fill_by_box_value_pairs(((box, value) for box in boxes), mode=mode, keep_max_value=keep_max_value,
                                     keep_min_value=keep_min_value, skip_values_uniqueness_check=True)

    def fill_by_polygon_value_pairs(self, polygon_value_pairs, mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                    keep_max_value: bool = False, keep_min_value: bool = False,
                                    skip_values_uniqueness_check: bool = False):
        self._fill_by_pairs(_sets.POLYGONS, polygon_value_pairs, mode, keep_max_value, keep_min_value,
                            skip_values_uniqueness_check)

    def fill_by_polygons(self, polygons: Iterable['Polygon'], value: Union['ScoreMap', np.ndarray, float] = 1.0,
                         mode: ElementSetOperationMode = ElementSetOperationMode.UNION, keep_max_value: bool = False,
                         keep_min_value: bool = False):
        self.fill_by_polygon_value_pairs(((polygon, value) for polygon in polygons), mode=mode, keep_max_value=keep_max_value,
                                         keep_min_value=keep_min_value, skip_values_uniqueness_check=True)

    def fill_by_mask_value_pairs(self, mask_value_pairs, mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                 keep_max_value: bool = False, keep_min_value: bool = False,
                                 skip_values_uniqueness_check: bool = False):
        self._fill_by_pairs(_sets.MASKS, mask_value_pairs, mode, keep_max_value, keep_min_value, skip_values_uniqueness_check)

    def fill_by_masks(self, masks: Iterable['Mask'], value: Union['ScoreMap', np.ndarray, float] = 1.0,
                      mode: ElementSetOperationMode = ElementSetOperationMode.UNION, keep_max_value: bool = False,
                      keep_min_value: bool = False):
        self.fill_by_mask_value_pairs(((mask, value) for mask in masks), mode=mode, keep_max_value=keep_max_value,
                                      keep_min_value=keep_min_value, skip_values_uniqueness_check=True)

    def __setitem__(self, element, config):
        """score_map[box | polygon | mask] = value | ScoreMapSetItemConfig (reference score_map.py:521-550)."""
        if isinstance(config, ScoreMapSetItemConfig):
            value, keep_max_value, keep_min_value = config.value, config.keep_max_value, config.keep_min_value
        else:
            value, keep_max_value, keep_min_value = config, False, False
        element.fill_score_map(score_map=self, value=value, keep_min_value=keep_min_value, keep_max_value=keep_max_value)

    def __getitem__(self, element):
        return element.extract_score_map(self)

    # ---- quad interpolation (reference score_map.py:139-283, :562-588): csrc/quad_interp.hip
    @classmethod
    def from_quad_interpolation(cls, point0: 'Point', point1: 'Point', point2: 'Point', point3: 'Point',
                                func_np_uv_to_mat: Callable[[np.ndarray], np.ndarray], is_prob: bool = True):
        """The inverse bilinear map of the quad point0 (u 0, v 0), point1 (u 1, v 0), point2 (u 1, v 1), point3 (u 0, v 1) over
        its bounding box, computed on the device; ``func_np_uv_to_mat`` takes the float32 (h, w, 2) array of (u, v).  With
        ``quad_u`` / ``quad_v`` are the callables the reference's callers write as lambdas."""
        record = _native.quad_records([(point0, point1, point2, point3)], _native.QUAD_V)
        mat = func_np_uv_to_mat(_native.quad_interp_uv(record).host())
        return cls(mat=mat, box=Polygon.create((point0, point1, point2, point3)).bounding_box, is_prob=is_prob)

    def fill_by_quad_interpolation(self, point0: 'Point', point1: 'Point', point2: 'Point', point3: 'Point',
                                   func_np_uv_to_mat: Callable[[np.ndarray], np.ndarray], keep_max_value: bool = False,
                                   keep_min_value: bool = False):
        """``from_quad_interpolation`` filled where it is > 0 (the destination's own box is not consulted: the quad's bounding box
        addresses the array, as in the reference).  With ``quad_u`` / ``quad_v`` the whole operation stays on the device."""
        if func_np_uv_to_mat is quad_u or func_np_uv_to_mat is quad_v:
            self.fill_by_quad_interpolations([(point0, point1, point2, point3)], func_np_uv_to_mat, keep_max_value=keep_max_value,
                                             keep_min_value=keep_min_value)
            return
        score_map = self.from_quad_interpolation(point0, point1, point2, point3, func_np_uv_to_mat, is_prob=self.is_prob)
        assert score_map.box
        fill = _sets._Fill(self, keep_max_value, keep_min_value)
        box = score_map.box
        if self.box:        # (_Fill addresses through the destination's box)
            box = box.to_shifted_box(offset_y=self.box.up, offset_x=self.box.left)
        fill.add(box, score_map.mat, mask=(score_map.mat > 0.0))
        fill.commit()

    def fill_by_quad_interpolations(self, quads, selector, keep_max_value: bool = False, keep_min_value: bool = False,
                                    zero_where=None):
        """``fill_by_quad_interpolation`` of every (point0, point1, point2, point3) of ``quads`` in list order with ``selector``
        (``quad_u`` / ``quad_v``, one or one a quad) in ONE device call of at most two launches.  ``zero_where``: a Mask (or uint8
        plane) of the destination's shape; where it is 0 the destination is 0.0 after the fills."""
        assert not (keep_max_value and keep_min_value)
        quads = list(quads)
        selectors = [selector] * len(quads) if callable(selector) else list(selector)
        assert len(selectors) == len(quads)
        components = []
        for one in selectors:
            if one is not quad_u and one is not quad_v:
                raise NotImplementedError('fill_by_quad_interpolations takes the selectors quad_u and quad_v')
            components.append(_native.QUAD_U if one is quad_u else _native.QUAD_V)
        records = _native.quad_records(quads, components)
        mode = _native.FILL_KEEP_MAX if keep_max_value else (_native.FILL_KEEP_MIN if keep_min_value else _native.FILL_PLAIN)
        if isinstance(zero_where, Mask):
            zero_where = zero_where._mat
        if isinstance(zero_where, np.ndarray) and zero_where.dtype == np.bool_:
            zero_where = zero_where.view(np.uint8)
        target = self._mat
        if isinstance(target, _native.DevArray):
            _native.quad_interp_fill(target, records, mode, None if zero_where is None else target.ctx.to_device(zero_where))
            return
        # a host destination is staged for the call and comes back on the host
        ctx = zero_where.ctx if isinstance(zero_where, _native.DevArray) else _native.default_ctx()
        staged = ctx.to_device(target)
        _native.quad_interp_fill(staged, records, mode, None if zero_where is None else ctx.to_device(zero_where))
        with self.writable_context:
            np.copyto(self._mat, staged.host())

    def to_shifted_score_map(self, offset_y: int = 0, offset_x: int = 0):
        assert self.box
        return attrs.evolve(self, box=self.box.to_shifted_box(offset_y=offset_y, offset_x=offset_x))

    def to_resized_score_map(self, resized_height: Optional[int] = None, resized_width: Optional[int] = None,
                             cv_resize_interpolation: int = 2):
        """cv.resize (any cv2 code 0..6), clipped back to [0, 1] for probability maps (reference score_map.py:616-637)."""
        assert not self.box
        if cv_resize_interpolation not in range(7):
            raise ValueError(f'unknown cv2 interpolation code {cv_resize_interpolation}')
        _, _, resized_height, resized_width = generate_shape_and_resized_shape(
            shapable_or_shape=self.shape, resized_height=resized_height, resized_width=resized_width)
        mat = _native.resize(self.arr, (resized_height, resized_width), cv_resize_interpolation)
        if self.is_prob:
            mat = np.clip(_native.host_array(mat), 0.0, 1.0)
        return attrs.evolve(self, mat=mat)

    def to_cropped_score_map(self, up=None, down=None, left=None, right=None):
        assert not self.box
        up = up or 0
        down = down or self.height - 1
        left = left or 0
        right = right or self.width - 1
        return attrs.evolve(self, mat=self.mat[up:down + 1, left:right + 1])

    def to_box_attached(self, box: 'Box'):
        assert self.height == box.height and self.width == box.width
        return attrs.evolve(self, box=box)

    def to_box_detached(self):
        assert self.box
        return attrs.evolve(self, box=None)

    def to_mask(self, threshold: float = 0.0):
        return Mask(mat=(self.mat > threshold).astype(np.uint8), box=self.box)

    # self is both the selection (alpha > 0) and the weight
    def fill_np_array(self, mat: np.ndarray, value, keep_max_value: bool = False, keep_min_value: bool = False):
        self.equivalent_box.fill_np_array(mat, value, alpha=self, keep_max_value=keep_max_value,
                                          keep_min_value=keep_min_value)

    def fill_image(self, image: 'Image', value):
        # The text lines of a page: a box-attached probability map and a constant colour recorded by an open deferred
        # composite on a uint8 image.  Same layer as the generic path below records (box geometry, the map as alpha plane,
        # no selection plane), without its five calls per layer.
        box, target, alpha = self.box, image._mat, self._mat
        if (box is not None and image.box is None and type(value) is tuple and self.is_prob and isinstance(alpha, (np.ndarray, _native.DevArray))
                and target.dtype == np.uint8 and target.ndim == 3 and len(value) == target.shape[2]):
            stack = _deferred_stack()
            if (stack and stack[-1].base is target and 0 <= box.up <= box.down < target.shape[0]
                    and 0 <= box.left <= box.right < target.shape[1]):
                stack[-1].layers.append(_native.make_layer((box.up, box.left, alpha.shape[0], alpha.shape[1]), len(value), value,
                                                           alpha=alpha))
                return
        self.equivalent_box.fill_image(image, value, alpha=self)


def generate_fill_by_score_maps_mask(shape, score_maps, mode: ElementSetOperationMode):
    if mode == ElementSetOperationMode.UNION:
        return None
    return Mask.from_score_maps(shape, score_maps, mode)


from .box import Box  # noqa: E402
from .mask import Mask  # noqa: E402
from .image import Image  # noqa: E402
from .point import Point  # noqa: E402,F401
from .polygon import Polygon  # noqa: E402
from . import _sets  # noqa: E402
