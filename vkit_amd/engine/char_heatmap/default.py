"""The default char-heatmap engine (reference: engine/char_heatmap/default.py): a Gaussian template warped into every char
quad, kept as the max and the min over the char's fillPoly raster, and mixed where chars overlap.  All chars of a call are
rasterised on the device by vkx_char_heatmap_fresh_dev (csrc/char_heatmap.hip): three launches and no synchronisation,
whatever the char count.

The template is computed here with numpy, by the reference's own expression, and uploaded with the call.  The exception the
reference raises for the first char whose box is not inside the page is raised here before any launch, from the boxes the
host computes itself.  A quad without 4 points or with a non-finite coordinate is refused with ValueError (the reference
fails inside OpenCV with cv2.error).

Every returned plane is proven to lie in [0, 1] for the configs the constructor accepts (char heatmap), so the
score maps of a device-resident page are built without the range scan that would download them."""
import math
from typing import Any, Mapping, Optional, Union

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Mask, ScoreMap
from vkit_amd.engine.char_mask.external_ellipse import char_quads
from .type import CharHeatmap, CharHeatmapEngineRunConfig

_MAX_RADIUS = 1024
_MAX_SIDE = 1 << 24


def build_np_distance(radius: int):
    # Make it symmetric.
    side_length = radius * 2 + 1

    # Build distances to the center point.
    np_offset = np.abs(np.arange(side_length, dtype=np.float32) - radius)
    np_vert_offset = np.repeat(np_offset[:, None], side_length, axis=1)
    np_hori_offset = np.repeat(np_offset[None, :], side_length, axis=0)
    np_distance = np.sqrt(np.square(np_vert_offset) + np.square(np_hori_offset))

    return np_distance


@attrs.define
class CharHeatmapDefaultEngineInitConfig:
    gaussian_map_distance_factor: float = 2.25
    gaussian_map_char_radius: int = 25
    gaussian_map_preserving_score_min: float = 0.9
    weight_neutralized_score_map: float = 0.4


@attrs.define
class CharHeatmapDefaultDebug:
    score_map_max: ScoreMap
    score_map_min: ScoreMap
    char_overlapped_mask: Mask
    char_neutralized_score_map: ScoreMap
    neutralized_mask: Mask
    neutralized_score_map: ScoreMap


def score_weights(weight: float):
    """float32(1 - w) (the difference in double, as Python computes it) and float32(w)."""
    return np.float32(1 - weight), np.float32(weight)


def weight_in_range(weight: float) -> bool:
    """True when score = f32(1 - w) * max + f32(w) * nscore stays in [0, 1] for every max, nscore in [0, 1]: both weights
    >= 0, and their float32 sum (the score at max = nscore = 1, its largest value: rounding is monotone) <= 1."""
    if not (isinstance(weight, (int, float, np.floating, np.integer)) and not isinstance(weight, bool)):
        return False
    weight = float(weight)
    if not (0.0 <= weight <= 1.0):
        return False
    a, b = score_weights(weight)
    return bool(a >= 0 and b >= 0 and np.float32(a + b) <= np.float32(1.0))


def _prob_score_map(arr):
    if isinstance(arr, np.ndarray):
        return ScoreMap(mat=arr)
    # a device plane: the range scan would download it; the range is proven instead (module docstring)
    score_map = ScoreMap(mat=arr, is_prob=False)
    object.__setattr__(score_map, 'is_prob', True)
    return score_map


def _box_exception(up, down, left, right, height, width):
    """The exception the reference raises for a char whose box is not inside the page: Box.extract_np_array asserts
    0 <= up <= down <= height (and the same for x); a box ending exactly at height / width passes it and leaves the extracted
    page one row / column short, which Box.prep_mat_and_value asserts against -- unless the box has the page's shape, when
    the value is cut the same way and the char's fillPoly mask no longer indexes it (IndexError in opt.fill_np_array)."""
    if not (0 <= up <= down <= height and 0 <= left <= right <= width):
        return AssertionError()
    if (down - up + 1, right - left + 1) == (height, width):
        return IndexError('boolean index did not match indexed array')
    return AssertionError()


class CharHeatmapDefaultEngine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'default'

    def __init__(self, init_config: CharHeatmapDefaultEngineInitConfig, init_resource=None):
        self.init_config = init_config
        radius = init_config.gaussian_map_char_radius
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= _MAX_RADIUS:
            raise ValueError('gaussian_map_char_radius must be an int in 1 .. 1024')
        factor = init_config.gaussian_map_distance_factor
        if not (isinstance(factor, (int, float, np.floating, np.integer)) and not isinstance(factor, bool)
                and math.isfinite(factor) and abs(factor) <= float(np.finfo(np.float32).max) and np.float32(factor) != 0):
            raise ValueError('gaussian_map_distance_factor must be finite and non-zero in float32')
        preserving = init_config.gaussian_map_preserving_score_min
        if not (isinstance(preserving, (int, float, np.floating, np.integer)) and not isinstance(preserving, bool)
                and math.isfinite(preserving) and abs(preserving) <= float(np.finfo(np.float32).max)):
            raise ValueError('gaussian_map_preserving_score_min must be finite in float32')
        if not weight_in_range(init_config.weight_neutralized_score_map):
            raise ValueError('weight_neutralized_score_map must be in [0, 1], with f32(1 - w) + f32(w) <= 1')
        self.np_gaussian_map, self.np_char_points = self.generate_np_gaussian_map()
        if not (np.isfinite(self.np_gaussian_map).all() and self.np_gaussian_map.min() >= 0
                and self.np_gaussian_map.max() <= 1):
            raise ValueError('the Gaussian template leaves [0, 1]')

    def generate_np_gaussian_map(self):
        char_radius = self.init_config.gaussian_map_char_radius
        np_distance = build_np_distance(char_radius)
        side_length = np_distance.shape[0]

        np_norm_distance = np_distance / char_radius
        np_gaussian_map = np.exp(-0.5 * np.square(self.init_config.gaussian_map_distance_factor * np_norm_distance))

        char_begin = 0
        char_end = side_length - 1
        np_char_src_points = np.asarray(
            [(char_begin, char_begin), (char_end, char_begin), (char_end, char_end), (char_begin, char_end)],
            dtype=np.float32,
        )
        return np_gaussian_map, np_char_src_points

    def run(self, run_config: CharHeatmapEngineRunConfig, rng: Optional[RandomGenerator] = None) -> CharHeatmap:
        height, width = int(run_config.height), int(run_config.width)
        if not (1 <= height < _MAX_SIDE and 1 <= width < _MAX_SIDE and height * width < (1 << 31)):
            raise ValueError('page shape out of range')
        try:
            quads = char_quads(run_config.char_polygons)
        except AssertionError:
            raise ValueError('a char polygon must have exactly 4 points') from None
        if not np.isfinite(quads).all():
            raise ValueError('non-finite char point')
        # Polygon.bounding_box: the rounded points' extent (round half to even, as Python's round)
        points = np.rint(quads)
        up, down = points[:, :, 1].min(axis=1), points[:, :, 1].max(axis=1)
        left, right = points[:, :, 0].min(axis=1), points[:, :, 0].max(axis=1)
        outside = np.nonzero((up < 0) | (down > height - 1) | (left < 0) | (right > width - 1))[0]
        if outside.size:
            k = int(outside[0])
            raise _box_exception(int(up[k]), int(down[k]), int(left[k]), int(right[k]), height, width)

        shape = (height, width)
        if _native.resident_mode():
            ctx = _native.default_ctx()
            new = lambda dtype: ctx.dev_empty(shape, dtype)      # noqa: E731
        else:
            new = lambda dtype: np.empty(shape, dtype)           # noqa: E731
        score = new(np.float32)
        debug_planes = None
        if run_config.enable_debug:
            debug_planes = {name: new(dtype) for name, dtype in _native.CHAR_HEATMAP_DEBUG_PLANES}
        config = self.init_config
        weight_max, weight_neutralized = score_weights(config.weight_neutralized_score_map)
        _native.char_heatmap(config.gaussian_map_char_radius, self.np_gaussian_map,
                             np.float32(config.gaussian_map_preserving_score_min), weight_max, weight_neutralized, quads,
                             shape, score, debug_planes)
        debug = None
        if debug_planes is not None:
            debug = CharHeatmapDefaultDebug(
                score_map_max=_prob_score_map(debug_planes['score_map_max']),
                score_map_min=_prob_score_map(debug_planes['score_map_min']),
                char_overlapped_mask=Mask(mat=debug_planes['char_overlapped_mask']),
                char_neutralized_score_map=_prob_score_map(debug_planes['char_neutralized_score_map']),
                neutralized_mask=Mask(mat=debug_planes['neutralized_mask']),
                neutralized_score_map=_prob_score_map(debug_planes['neutralized_score_map']),
            )
        return CharHeatmap(score_map=_prob_score_map(score), debug=debug)


class CharHeatmapEngineExecutor:
    """``run`` takes a CharHeatmapEngineRunConfig or the mapping of its fields, as the reference's EngineExecutor does."""

    def __init__(self, engine):
        self.engine = engine

    def run(self, run_config: Union[CharHeatmapEngineRunConfig, Mapping[str, Any]], rng=None) -> CharHeatmap:
        if not isinstance(run_config, CharHeatmapEngineRunConfig):
            run_config = CharHeatmapEngineRunConfig(**run_config)
        return self.engine.run(run_config, rng)


class CharHeatmapEngineExecutorFactory:
    """The slice of the reference's EngineExecutorFactory (engine/interface.py:123-190) this engine uses: ``create`` takes an
    init config, the mapping of its fields or None (the defaults)."""

    def __init__(self, engine_cls, init_config_cls):
        self.engine_cls, self.init_config_cls = engine_cls, init_config_cls

    def get_type_name(self):
        return self.engine_cls.get_type_name()

    def get_init_config_cls(self):
        return self.init_config_cls

    def create(self, init_config: Optional[Union[Mapping[str, Any], CharHeatmapDefaultEngineInitConfig]] = None,
               init_resource: Optional[Any] = None) -> CharHeatmapEngineExecutor:
        if init_config is None:
            init_config = self.init_config_cls()
        elif not isinstance(init_config, self.init_config_cls):
            if not isinstance(init_config, Mapping):
                raise TypeError('init_config: an init config, a mapping of its fields or None')
            init_config = self.init_config_cls(**dict(init_config))
        return CharHeatmapEngineExecutor(self.engine_cls(init_config, init_resource))


char_heatmap_default_engine_executor_factory = CharHeatmapEngineExecutorFactory(CharHeatmapDefaultEngine,
                                                                                CharHeatmapDefaultEngineInitConfig)
