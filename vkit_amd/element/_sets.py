"""The ``fill_by_*`` families of Image / Mask / ScoreMap and the ``Mask.from_*`` constructors behind them (reference:
vkit/element/image.py:371-665, mask.py:174-244,283-410, score_map.py:315-520), stated once for the three destinations.

The reference walks the list: one count pass an element for the set mask, one ``fill_*`` an element for the fill.  Here the set
mask of the whole list -- and the polygons' own rasters -- come from ONE ``_native.set_mask`` call (csrc/element_sets.hip, at
most four launches), and the fills of the whole list are layers of ONE composite call: an open ``deferred_fill`` on the
destination takes them, else the list is its own call.  The control flow is the reference's, quirks included:

UNION                       the elements in list order, later ones over earlier ones, each with its own value (and alpha).
DISTINCT / INTERSECT,       one fill of ``values[0]`` (``alphas[0]``; for score maps ``score_maps[0]``) under the set mask.
unique values
DISTINCT / INTERSECT,       per element, in order, the window of the set mask over the element's box -- for a polygon its
non-unique values           BOUNDING box, so pixels of the set mask that belong to another polygon are filled too -- and for
                            masks and score maps that window ANDed with the element's own active pixels and, the window
                            having lost its box in the reference, filled at the destination's ORIGIN.
"""
import numpy as np

from vkit_amd import _native

from .opt import _deferred_stack
from .type import ElementSetOperationMode
from .uniqueness import check_elements_uniqueness

BOXES, POLYGONS, MASKS, SCORE_MAPS = 'boxes', 'polygons', 'masks', 'score_maps'


def unpack_shape_or_box(shape_or_box):
    if isinstance(shape_or_box, Box):
        return shape_or_box.shape, shape_or_box
    return tuple(shape_or_box), None


def set_entries(kind, elements, origin=None):
    """The elements as ``_native.set_mask`` takes them, relative to the box ``origin``."""
    oy, ox = (origin.up, origin.left) if origin else (0, 0)
    entries = []
    for element in elements:
        if kind == BOXES:
            entries.append(element.to_relative_box(origin_y=oy, origin_x=ox) if origin else element)
        elif kind == POLYGONS:
            table = element.to_np_array()
            entries.append(table - np.array([ox, oy], np.int32) if origin else table)
        elif element.box and origin and not (origin.up <= element.box.up and element.box.down <= origin.down and
                                             origin.left <= element.box.left and element.box.right <= origin.right):
            # a plane that reaches beyond the box takes part with what lies inside it
            up, down = max(element.box.up, origin.up), min(element.box.down, origin.down)
            left, right = max(element.box.left, origin.left), min(element.box.right, origin.right)
            if up > down or left > right:
                raise ValueError('an element that lies outside the box altogether')
            entries.append((element.arr, (up - oy, left - ox),
                            (up - element.box.up, left - element.box.left, down - up + 1, right - left + 1)))
        elif element.box:
            entries.append((element.arr, (element.box.up - oy, element.box.left - ox)))
        else:
            entries.append(element.arr)
    return entries


def polygon_tables(polygons):
    """(the int32 (x, y) tables of the polygons, their bounding boxes): the boxes of the whole list from one pass over one
    table (``Polygon.bounding_box`` rounds the same integers; a polygon that has not computed its own takes this one)."""
    tables = [polygon.to_np_array() for polygon in polygons]
    if not tables:
        return tables, []
    flat = np.concatenate(tables)
    counts = np.fromiter((len(table) for table in tables), np.int64, len(tables))
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    lo, hi = np.minimum.reduceat(flat, starts, axis=0).tolist(), np.maximum.reduceat(flat, starts, axis=0).tolist()
    boxes = []
    for polygon, (left, up), (right, down) in zip(polygons, lo, hi):
        if polygon._bounding_box is None:
            object.__setattr__(polygon, '_bounding_box', Box(up=up, down=down, left=left, right=right))
        boxes.append(polygon._bounding_box)
    return tables, boxes


def build_set_mask(kind, shape_or_box, elements, mode, on_device=None, want_windows=False, gated=False, ctx=None, entries=None):
    """``Mask.from_<kind>``: (Mask, the elements' own windows or None).  ``entries``: the elements as ``set_entries`` gives them,
    where the caller has them already."""
    if not isinstance(mode, ElementSetOperationMode):
        raise NotImplementedError()
    shape, attached_box = unpack_shape_or_box(shape_or_box)
    if entries is None:
        entries = set_entries(kind, elements, attached_box)
    with _native.resident(_native.resident_mode() if on_device is None else on_device):
        out = _native.set_mask(entries, shape, mode, want_windows=want_windows, gated=gated, ctx=ctx)
    mat, windows = out if want_windows else (out, None)
    if on_device is False:            # (element planes on the device, a destination on the host)
        mat = _native.host_array(mat)
        windows = windows and [_native.host_array(window) for window in windows]
    return Mask(mat=mat, box=attached_box), windows


def _window(plane, up, left, height, width):
    """(address, row step, keepalive) of a window of the uint8 plane ``plane`` (numpy or DevArray)."""
    if isinstance(plane, _native.DevArray):
        view = _native.DevView(plane, up * plane.shape[1] + left, (1, width))
        return view.ptr, plane.shape[1], [plane, view]
    view = plane[up:up + height, left:left + width]
    return view.ctypes.data, plane.strides[0], [plane, view]


class _Fill:
    """The layers of one ``fill_by_*`` call on ``dest``."""

    def __init__(self, dest, keep_max_value=False, keep_min_value=False):
        self.dest, self.target = dest, dest._mat
        self.dtype = np.dtype(self.target.dtype)
        if self.dtype not in (np.uint8, np.float32) or (self.dtype == np.float32 and self.target.ndim != 2):
            raise NotImplementedError(f'fill_by_* on a {self.dtype} array of {self.target.ndim} dimensions is outside the accelerated path.')
        self.cn = 1 if self.target.ndim == 2 else self.target.shape[2]
        self.value_cls = type(dest)
        self.mode = _native.FILL_PLAIN
        if keep_max_value or keep_min_value:
            assert not (keep_max_value and keep_min_value)
            self.mode = _native.FILL_KEEP_MAX if keep_max_value else _native.FILL_KEEP_MIN
        self.on_device = isinstance(self.target, _native.DevArray)
        self.ctx = self.target.ctx if self.on_device else None
        self.layers = []

    def add(self, box, value, alpha=1.0, mask=None, window_of=None):
        """One element: ``box`` in the destination's coordinates; ``mask`` a dense uint8 / bool plane of the box's shape, or
        ``window_of`` the uint8 plane of the destination's shape whose window over the box selects the pixels."""
        relative_box, _ = box.get_boxes_for_box_attached_opt(self.dest.box)
        assert 0 <= relative_box.up <= relative_box.down < self.target.shape[0]
        assert 0 <= relative_box.left <= relative_box.right < self.target.shape[1]
        shape = box.shape
        if isinstance(value, self.value_cls):
            value = value._mat if value.shape == shape else box._extract_element(value).mat
        if isinstance(value, np.ndarray):
            if tuple(value.shape[:2]) != shape:
                assert tuple(value.shape[:2]) == tuple(self.target.shape[:2])
                value = relative_box.extract_np_array(value)
            if value.dtype != self.dtype:
                value = value.astype(self.dtype)
        elif self.target.ndim == 2 and isinstance(value, tuple):
            raise ValueError('a tuple value needs a 3-D destination')
        if isinstance(alpha, ScoreMap):
            assert alpha.is_prob     # ScoreMap.box is ignored
            alpha = alpha._mat
        if not isinstance(alpha, (float, np.ndarray, _native.DevArray)):
            raise AttributeError(f'alpha must be a float or a numpy array, got {type(alpha).__name__}')
        selected = mask is not None or window_of is not None
        if isinstance(alpha, float):
            if alpha < 0.0 or alpha > 1.0:
                raise RuntimeError(f'alpha={alpha} is invalid.')
            if 0.0 < alpha < 1.0 and selected and self.target.ndim == 2:
                raise IndexError('tuple index out of range')        # the reference's own failure (vkit/element/opt.py:172-176)
        if isinstance(mask, np.ndarray) and mask.dtype == np.bool_:
            mask = mask.view(np.uint8)
        if not self.on_device:           # a host destination takes host planes
            value, alpha, mask, window_of = (_native.host_array(plane) if isinstance(plane, _native.DevArray) else plane
                                             for plane in (value, alpha, mask, window_of))
        layer, keep = _native.make_layer((relative_box.up, relative_box.left) + shape, self.cn, value, mask=mask, alpha=alpha,
                                         mode=self.mode, dtype=self.dtype)
        if window_of is not None:
            assert tuple(window_of.shape) == tuple(self.target.shape[:2])
            layer.mask, layer.mask_stride, planes = _window(window_of, relative_box.up, relative_box.left, *shape)
            keep = keep + planes
        self.layers.append((layer, keep))

    def commit(self):
        if not self.layers:
            return
        if isinstance(self.dest, Mask):
            self.dest.set_np_mask_out_of_date()
        stack = _deferred_stack()
        if stack and stack[-1].base is self.target:
            stack[-1].layers.extend(self.layers)       # the open composite on this destination writes on its exit
            return
        if self.on_device:
            _native.fill(self.target, self.layers)
            return
        with self.dest.writable_context:       # (may replace a read-only view by a copy)
            mat = self.dest._mat
            if mat.flags.c_contiguous:
                _native.fill(mat, self.layers)
            else:
                packed = np.ascontiguousarray(mat)
                _native.fill(packed, self.layers)
                mat[...] = packed


def fill_by(dest, kind, elements, values, alphas, mode, keep_max_value=False, keep_min_value=False,
            skip_values_uniqueness_check=False):
    """``dest.fill_by_<kind>_value_{pairs,tuples}`` after unpacking.  ``alphas``: one an element (None: 1.0 each; ignored for
    score maps, which are their own alpha)."""
    if not isinstance(mode, ElementSetOperationMode):
        raise NotImplementedError()
    elements, values = list(elements), list(values)
    alphas = [1.0] * len(elements) if alphas is None else list(alphas)
    if kind == SCORE_MAPS:
        alphas = list(elements)
    fill = _Fill(dest, keep_max_value, keep_min_value)
    if kind == BOXES:
        boxes, tables = elements, None
    elif kind == POLYGONS:
        tables, boxes = polygon_tables(elements)
    else:
        boxes, tables = [element.box or Box.from_shape(dest.shape) for element in elements], None

    if mode == ElementSetOperationMode.UNION:
        rasters = [None] * len(elements)
        if kind == POLYGONS and elements:
            # the rasters of all polygons from one call (the set mask it also builds is not used)
            if dest.box:       # the destination's own coordinates
                tables = [table - np.array([dest.box.left, dest.box.up], np.int32) for table in tables]
            _, rasters = build_set_mask(POLYGONS, dest.shape, elements, mode, on_device=fill.on_device, want_windows=True,
                                        ctx=fill.ctx, entries=tables)
        elif kind == MASKS:
            rasters = [mask._mat for mask in elements]
        for box, value, alpha, raster in zip(boxes, values, alphas, rasters):
            fill.add(box, value, alpha=alpha, mask=raster)
        fill.commit()
        return

    unique = skip_values_uniqueness_check or (
        check_elements_uniqueness(values) and (kind == SCORE_MAPS or check_elements_uniqueness(alphas)))
    own = not unique and kind in (MASKS, SCORE_MAPS)
    set_mask, windows = build_set_mask(kind, dest.shape, elements, mode, on_device=fill.on_device, want_windows=own, gated=own,
                                       ctx=fill.ctx, entries=tables)
    if unique:
        fill.add(Box.from_shape(dest.shape), values[0], alpha=alphas[0], mask=set_mask._mat)
    elif own:
        # (the reference extracts the window of the set mask WITHOUT its box, mask.box.extract_mask(masks_mask) on a mask that has
        #  none, and fills through it as it is: at the destination's origin, not at the element's box; image.py:579-591,641-653)
        for element, value, alpha, window in zip(elements, values, alphas, windows):
            fill.add(Box.from_shape(element.shape), value, alpha=alpha, mask=window)
    else:
        for box, value, alpha in zip(boxes, values, alphas):
            fill.add(box, value, alpha=alpha, window_of=set_mask._mat)
    fill.commit()


def unpack_element_value_pairs(element_value_pairs):
    elements, values = [], []
    for element, value in element_value_pairs:
        elements.append(element)
        values.append(value)
    return elements, values


from .box import Box  # noqa: E402
from .mask import Mask  # noqa: E402
from .score_map import ScoreMap  # noqa: E402
