"""The ``ellipse`` seal-impression engine (reference: vkit/engine/seal_impression/ellipse.py): an elliptic border, optionally a
double line, an optional icon in the middle, one or two curved text lines of char slots along the border and an optional box
for a straight text line inside.

Everything that is sampled is sampled on the host and consumes the generator exactly as the reference does, draw for draw and
in its order: alpha and colour, the rough placement of the curved text lines, per text line its char aspect ratio, char spacing
and the coin for the last out-of-bound slot, then in ``generate_background`` the border style and thickness, the width of a
double line's gap, the icon coin, the icon box and the icon file, the internal text line coin and its box.  ``sample_background``
is that host half of ``generate_background``; ``draw_background`` is the device half: the border is a thick ellipse outline on
a fresh mask (``vkx_ellipse_mask_u8_dev``); the gap of a double line is the same outline drawn on a scratch plane and cleared
from the mask by one composite layer -- the pixels cv.ellipse touches do not depend on the colour --; the icon is the selector
image engine's grayscale image thresholded by a table look-up and copied into its box."""
from ctypes import c_void_p
from enum import Enum, unique
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Box, ImageMode, Mask, Point, PointList
from vkit_amd.engine.image import image_selector_engine_executor_factory
from vkit_amd.utility import normalize_to_probs, rng_choice
from ..interface import EngineExecutorFactory, NoneTypeEngineInitResource
from .type import CharSlot, SealImpression, SealImpressionEngineRunConfig, TextLineSlot


@attrs.define
class SealImpressionEllipseEngineInitConfig:
    # Color & Transparency.
    color_rgb_min: int = 128
    color_rgb_max: int = 255
    weight_color_grayscale: float = 5
    weight_color_red: float = 10
    weight_color_green: float = 1
    weight_color_blue: float = 1
    alpha_min: float = 0.25
    alpha_max: float = 0.75

    # Border.
    border_thickness_ratio_min: float = 0.0
    border_thickness_ratio_max: float = 0.03
    border_thickness_min: int = 2
    weight_border_style_solid_line: float = 3
    weight_border_style_double_lines: float = 1

    # Char slots.  NOTE: the ratios are relative to the height of the seal impression.
    pad_ratio_min: float = 0.03
    pad_ratio_max: float = 0.08
    text_line_height_ratio_min: float = 0.075
    text_line_height_ratio_max: float = 0.2
    weight_text_line_mode_one: float = 1
    weight_text_line_mode_two: float = 1
    text_line_mode_one_gap_ratio_min: float = 0.1
    text_line_mode_one_gap_ratio_max: float = 0.55
    text_line_mode_two_gap_ratio_min: float = 0.1
    text_line_mode_two_gap_ratio_max: float = 0.4
    char_aspect_ratio_min: float = 0.4
    char_aspect_ratio_max: float = 0.9
    char_space_ratio_min: float = 0.05
    char_space_ratio_max: float = 0.25
    angle_step_min: int = 10

    # Icon.
    icon_image_folders: Optional[Sequence[str]] = None
    icon_image_grayscale_min: int = 127
    prob_add_icon: float = 0.9
    icon_height_ratio_min: float = 0.35
    icon_height_ratio_max: float = 0.75
    icon_width_ratio_min: float = 0.35
    icon_width_ratio_max: float = 0.75

    # Internal text line.
    prob_add_internal_text_line: float = 0.5
    internal_text_line_height_ratio_min: float = 0.075
    internal_text_line_height_ratio_max: float = 0.15
    internal_text_line_width_ratio_min: float = 0.22
    internal_text_line_width_ratio_max: float = 0.5


@unique
class SealImpressionEllipseBorderStyle(Enum):
    SOLID_LINE = 'solid_line'
    DOUBLE_LINES = 'double_lines'


@unique
class SealImpressionEllipseTextLineMode(Enum):
    ONE = 'one'
    TWO = 'two'


@unique
class SealImpressionEllipseColorMode(Enum):
    GRAYSCALE = 'grayscale'
    RED = 'red'
    GREEN = 'green'
    BLUE = 'blue'


@attrs.define
class TextLineRoughPlacement:
    ellipse_outer_height: int
    ellipse_outer_width: int
    ellipse_inner_height: int
    ellipse_inner_width: int
    text_line_height: int
    angle_begin: int
    angle_end: int
    clockwise: bool


@attrs.define
class SealImpressionEllipseBackground:
    """What ``sample_background`` drew: all that ``draw_background`` needs, and the box of the internal text line."""
    border_style: SealImpressionEllipseBorderStyle
    border_thickness: int
    center: Tuple[int, int]
    axes: Tuple[int, int]
    border_thickness_empty: Optional[int]
    icon_box: Optional[Box]
    icon_grayscale_image: Optional[object]
    internal_text_line_box: Optional[Box]


def _keys_and_probs(pairs):
    return [key for key, _ in pairs], normalize_to_probs([weight for _, weight in pairs])


class SealImpressionEllipseEngine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'ellipse'

    def __init__(self, init_config: SealImpressionEllipseEngineInitConfig,
                 init_resource: Optional[NoneTypeEngineInitResource] = None):
        self.init_config = init_config
        self.init_resource = init_resource
        config = init_config
        self.border_styles, self.border_styles_probs = _keys_and_probs([
            (SealImpressionEllipseBorderStyle.SOLID_LINE, config.weight_border_style_solid_line),
            (SealImpressionEllipseBorderStyle.DOUBLE_LINES, config.weight_border_style_double_lines),
        ])
        self.text_line_modes, self.text_line_modes_probs = _keys_and_probs([
            (SealImpressionEllipseTextLineMode.ONE, config.weight_text_line_mode_one),
            (SealImpressionEllipseTextLineMode.TWO, config.weight_text_line_mode_two),
        ])
        self.color_modes, self.color_modes_probs = _keys_and_probs([
            (SealImpressionEllipseColorMode.GRAYSCALE, config.weight_color_grayscale),
            (SealImpressionEllipseColorMode.RED, config.weight_color_red),
            (SealImpressionEllipseColorMode.GREEN, config.weight_color_green),
            (SealImpressionEllipseColorMode.BLUE, config.weight_color_blue),
        ])
        self.icon_image_selector = None
        if config.icon_image_folders:
            self.icon_image_selector = image_selector_engine_executor_factory.create({
                'image_folders': config.icon_image_folders,
                'target_image_mode': ImageMode.GRAYSCALE,
                'force_resize': True,
            })

    # ---- host sampling ------------------------------------------------------------------------------------------
    def sample_alpha_and_color(self, rng: RandomGenerator):
        config = self.init_config
        alpha = float(rng.uniform(config.alpha_min, config.alpha_max))
        color_mode = rng_choice(rng, self.color_modes, probs=self.color_modes_probs)
        rgb_value = int(rng.integers(config.color_rgb_min, config.color_rgb_max + 1))
        channel = {SealImpressionEllipseColorMode.RED: 0, SealImpressionEllipseColorMode.GREEN: 1,
                   SealImpressionEllipseColorMode.BLUE: 2}
        if color_mode == SealImpressionEllipseColorMode.GRAYSCALE:
            color = (rgb_value,) * 3
        else:
            color = tuple(rgb_value if k == channel[color_mode] else 0 for k in range(3))
        return alpha, color

    @classmethod
    def sample_ellipse_points(cls, ellipse_height: int, ellipse_width: int, ellipse_offset_y: int, ellipse_offset_x: int,
                              angle_begin: int, angle_end: int, angle_step: int, keep_last_oob: bool):
        """The points of the ellipse at angle_begin, + angle_step, ... up to angle_end; ``keep_last_oob`` adds the first one
        past it."""
        points = PointList()
        half_ellipse_height = ellipse_height / 2
        half_ellipse_width = ellipse_width / 2
        angle = angle_begin
        while angle <= angle_end or (keep_last_oob and angle - angle_end < angle_step):
            theta = angle / 180 * np.pi
            x, y = float(np.cos(theta)), float(np.sin(theta))
            points.append(Point.create(y=y * half_ellipse_height + ellipse_offset_y, x=x * half_ellipse_width + ellipse_offset_x))
            angle += angle_step
        return points

    @classmethod
    def sample_char_slots(cls, ellipse_up_height: int, ellipse_up_width: int, ellipse_down_height: int, ellipse_down_width: int,
                          ellipse_offset_y: int, ellipse_offset_x: int, angle_begin: int, angle_end: int, angle_step: int,
                          rng: RandomGenerator, reverse: bool = False):
        keep_last_oob = (rng.random() < 0.5)
        shared = dict(ellipse_offset_y=ellipse_offset_y, ellipse_offset_x=ellipse_offset_x, angle_begin=angle_begin,
                      angle_end=angle_end, angle_step=angle_step, keep_last_oob=keep_last_oob)
        point_ups = cls.sample_ellipse_points(ellipse_height=ellipse_up_height, ellipse_width=ellipse_up_width, **shared)
        point_downs = cls.sample_ellipse_points(ellipse_height=ellipse_down_height, ellipse_width=ellipse_down_width, **shared)
        char_slots = [CharSlot.build(point_up=point_up, point_down=point_down) for point_up, point_down in zip(point_ups, point_downs)]
        if reverse:
            char_slots.reverse()
        return char_slots

    def sample_curved_text_line_rough_placements(self, height: int, width: int, rng: RandomGenerator):
        config = self.init_config
        # the outer ellipse, shared by the text lines
        pad_ratio = float(rng.uniform(config.pad_ratio_min, config.pad_ratio_max))
        pad = round(pad_ratio * height)
        ellipse_outer_height = height - 2 * pad
        ellipse_outer_width = width - 2 * pad
        assert ellipse_outer_height > 0 and ellipse_outer_width > 0

        text_line_mode = rng_choice(rng, self.text_line_modes, probs=self.text_line_modes_probs)
        half_gap = None
        if text_line_mode == SealImpressionEllipseTextLineMode.ONE:
            # one text line around the seal, its gap centred at the bottom
            gap_ratio = float(rng.uniform(config.text_line_mode_one_gap_ratio_min, config.text_line_mode_one_gap_ratio_max))
            angle_gap = round(gap_ratio * 360)
            angle_begin = 90 + angle_gap // 2
            angle_end = angle_begin + (360 - angle_gap) - 1
        elif text_line_mode == SealImpressionEllipseTextLineMode.TWO:
            # an upper and a lower text line with the gaps at the sides
            gap_ratio = float(rng.uniform(config.text_line_mode_two_gap_ratio_min, config.text_line_mode_two_gap_ratio_max))
            half_gap = round(gap_ratio * 360 / 2)
            angle_begin = 180 + half_gap
            angle_end = 360 - half_gap
        else:
            raise NotImplementedError()

        def placement(angle_begin, angle_end, clockwise):
            height_ratio = float(rng.uniform(config.text_line_height_ratio_min, config.text_line_height_ratio_max))
            text_line_height = round(height_ratio * height)
            assert text_line_height > 0
            ellipse_inner_height = ellipse_outer_height - 2 * text_line_height
            ellipse_inner_width = ellipse_outer_width - 2 * text_line_height
            assert ellipse_inner_height > 0 and ellipse_inner_width > 0
            return TextLineRoughPlacement(
                ellipse_outer_height=ellipse_outer_height, ellipse_outer_width=ellipse_outer_width,
                ellipse_inner_height=ellipse_inner_height, ellipse_inner_width=ellipse_inner_width,
                text_line_height=text_line_height, angle_begin=angle_begin, angle_end=angle_end, clockwise=clockwise)

        rough_placements: List[TextLineRoughPlacement] = [placement(angle_begin, angle_end, True)]
        if text_line_mode == SealImpressionEllipseTextLineMode.TWO:
            assert half_gap
            rough_placements.append(placement(half_gap, 180 - half_gap, False))
        return rough_placements

    def generate_text_line_slots_based_on_rough_placements(self, height: int, width: int,
                                                           rough_placements: Sequence[TextLineRoughPlacement],
                                                           rng: RandomGenerator):
        config = self.init_config
        ellipse_offset_y = height // 2
        ellipse_offset_x = width // 2
        text_line_slots: List[TextLineSlot] = []
        for rough_placement in rough_placements:
            char_aspect_ratio = float(rng.uniform(config.char_aspect_ratio_min, config.char_aspect_ratio_max))
            char_width_ref = max(1, round(rough_placement.text_line_height * char_aspect_ratio))
            char_space_ratio = float(rng.uniform(config.char_space_ratio_min, config.char_space_ratio_max))
            char_space_ref = max(1, round(rough_placement.text_line_height * char_space_ratio))
            radius_ref = max(1, ellipse_offset_y)
            angle_step = max(config.angle_step_min, round(360 * (char_width_ref + char_space_ref) / (2 * np.pi * radius_ref)))

            outer = (rough_placement.ellipse_outer_height, rough_placement.ellipse_outer_width)
            inner = (rough_placement.ellipse_inner_height, rough_placement.ellipse_inner_width)
            # clockwise: the chars stand on the inner ellipse; else they hang from it and are listed in reverse
            up, down = (outer, inner) if rough_placement.clockwise else (inner, outer)
            char_slots = self.sample_char_slots(
                ellipse_up_height=up[0], ellipse_up_width=up[1], ellipse_down_height=down[0], ellipse_down_width=down[1],
                ellipse_offset_y=ellipse_offset_y, ellipse_offset_x=ellipse_offset_x, angle_begin=rough_placement.angle_begin,
                angle_end=rough_placement.angle_end, angle_step=angle_step, rng=rng, reverse=not rough_placement.clockwise)
            text_line_slots.append(TextLineSlot(text_line_height=rough_placement.text_line_height,
                                                char_aspect_ratio=char_aspect_ratio, char_slots=char_slots))
        return text_line_slots

    def generate_text_line_slots(self, height: int, width: int, rng: RandomGenerator):
        rough_placements = self.sample_curved_text_line_rough_placements(height=height, width=width, rng=rng)
        text_line_slots = self.generate_text_line_slots_based_on_rough_placements(
            height=height, width=width, rough_placements=rough_placements, rng=rng)
        ellipse_inner_shape = (min(p.ellipse_inner_height for p in rough_placements),
                               min(p.ellipse_inner_width for p in rough_placements))
        return text_line_slots, ellipse_inner_shape

    def sample_icon_box(self, height: int, width: int, ellipse_inner_shape: Tuple[int, int], rng: RandomGenerator):
        config = self.init_config
        ellipse_inner_height, ellipse_inner_width = ellipse_inner_shape
        box_height = round(ellipse_inner_height * rng.uniform(config.icon_height_ratio_min, config.icon_height_ratio_max))
        box_width = round(ellipse_inner_width * rng.uniform(config.icon_width_ratio_min, config.icon_width_ratio_max))
        up = (height - box_height) // 2
        left = (width - box_width) // 2
        return Box(up=up, down=up + box_height - 1, left=left, right=left + box_width - 1)

    def sample_internal_text_line_box(self, height: int, width: int, ellipse_inner_shape: Tuple[int, int],
                                      icon_box_down: Optional[int], rng: RandomGenerator):
        config = self.init_config
        ellipse_inner_height, ellipse_inner_width = ellipse_inner_shape
        if ellipse_inner_height > ellipse_inner_width:
            return None         # not supported (by the reference either)

        # rows: below the icon (or the centre), inside the inner ellipse
        box_height = round(ellipse_inner_height * rng.uniform(config.internal_text_line_height_ratio_min,
                                                               config.internal_text_line_height_ratio_max))
        half_height = height // 2
        up = half_height
        if icon_box_down:
            up = icon_box_down + 1
        down = min(height - 1, half_height + ellipse_inner_height // 2 - 1, up + box_height - 1)
        if up > down:
            return None

        # columns: at least the chord of the inner ellipse at the box's last row
        ellipse_h = down + 1 - half_height
        ellipse_a = ellipse_inner_width / 2
        ellipse_b = ellipse_inner_height / 2
        box_width_max = round(2 * ellipse_b * np.sqrt(ellipse_a**2 - ellipse_h**2) / ellipse_a)
        box_width = round(ellipse_inner_width * rng.uniform(config.internal_text_line_width_ratio_min,
                                                             config.internal_text_line_width_ratio_max))
        box_width = max(box_width_max, box_width)
        left = (width - box_width) // 2
        right = left + box_width - 1
        if left > right:
            return None
        return Box(up=up, down=down, left=left, right=right)

    def sample_background(self, height: int, width: int, ellipse_inner_shape: Tuple[int, int], rng: RandomGenerator):
        """The host half of ``generate_background``: every draw of it, in the reference's order (the icon's file is drawn by
        the selector engine, which also produces the icon image)."""
        config = self.init_config
        border_style = rng_choice(rng, self.border_styles, probs=self.border_styles_probs)
        border_thickness_ratio = float(rng.uniform(config.border_thickness_ratio_min, config.border_thickness_ratio_max))
        border_thickness = max(config.border_thickness_min, round(height * border_thickness_ratio))
        center = (width // 2, height // 2)
        # NOTE: minus 1 to make sure the border is inbound.
        axes = (width // 2 - border_thickness - 1, height // 2 - border_thickness - 1)

        border_thickness_empty = None
        if border_thickness > 2 * config.border_thickness_min + 1 and border_style == SealImpressionEllipseBorderStyle.DOUBLE_LINES:
            # the middle part of the border is removed
            border_thickness_empty = int(rng.integers(1, border_thickness - 2 * config.border_thickness_min))

        icon_box = icon_grayscale_image = None
        if self.icon_image_selector and rng.random() < config.prob_add_icon:
            icon_box = self.sample_icon_box(height=height, width=width, ellipse_inner_shape=ellipse_inner_shape, rng=rng)
            icon_grayscale_image = self.icon_image_selector.run({'height': icon_box.height, 'width': icon_box.width}, rng)

        internal_text_line_box = None
        if rng.random() < config.prob_add_internal_text_line:
            internal_text_line_box = self.sample_internal_text_line_box(
                height=height, width=width, ellipse_inner_shape=ellipse_inner_shape,
                icon_box_down=icon_box.down if icon_box else None, rng=rng)
        return SealImpressionEllipseBackground(
            border_style=border_style, border_thickness=border_thickness, center=center, axes=axes,
            border_thickness_empty=border_thickness_empty, icon_box=icon_box, icon_grayscale_image=icon_grayscale_image,
            internal_text_line_box=internal_text_line_box)

    # ---- device drawing -----------------------------------------------------------------------------------------
    def draw_background(self, height: int, width: int, background: SealImpressionEllipseBackground) -> Mask:
        """The background mask of ``background`` on the device; a host array outside resident mode."""
        ctx = _native.default_ctx()
        axes = np.asarray([background.axes], np.int32)

        def outline(thickness):
            plane = _native.dev_zeros((height, width), np.uint8, ctx)
            _native.check(_native.lib().vkx_ellipse_mask_u8_dev(ctx.handle, c_void_p(plane.ptr), width, height, width,
                                                                background.center[0], background.center[1], axes.ctypes.data, 1,
                                                                int(thickness)))
            return plane

        mat = outline(background.border_thickness)
        if background.border_thickness_empty is not None:
            # cv.ellipse(..., color=0, ...): value 0 under the outline's own pixels
            _native.fill(mat, [_native.make_layer((0, 0, height, width), 1, 0, mask=outline(background.border_thickness_empty))])
        if background.icon_box is not None:
            icon_box = background.icon_box
            above = (np.arange(256) > self.init_config.icon_image_grayscale_min).astype(np.uint8).reshape(1, 256)
            icon_mask = _native.apply_lut(background.icon_grayscale_image.arr, above)
            # Box.fill_mask with a mask as the value: a plain copy into the box, its zeros included
            _native.fill(mat, [_native.make_layer((icon_box.up, icon_box.left, icon_box.height, icon_box.width), 1, icon_mask)])
        return Mask(mat=mat if _native.resident_mode() else np.array(mat.host()))

    def generate_background(self, height: int, width: int, ellipse_inner_shape: Tuple[int, int], rng: RandomGenerator):
        background = self.sample_background(height=height, width=width, ellipse_inner_shape=ellipse_inner_shape, rng=rng)
        return self.draw_background(height, width, background), background.internal_text_line_box

    def run(self, run_config: SealImpressionEngineRunConfig, rng: Optional[RandomGenerator] = None) -> SealImpression:
        assert rng is not None
        alpha, color = self.sample_alpha_and_color(rng)
        text_line_slots, ellipse_inner_shape = self.generate_text_line_slots(height=run_config.height, width=run_config.width, rng=rng)
        background_mask, internal_text_line_box = self.generate_background(
            height=run_config.height, width=run_config.width, ellipse_inner_shape=ellipse_inner_shape, rng=rng)
        return SealImpression(alpha=alpha, color=color, background_mask=background_mask, text_line_slots=text_line_slots,
                              internal_text_line_box=internal_text_line_box)


seal_impression_ellipse_engine_executor_factory = EngineExecutorFactory(
    SealImpressionEllipseEngine, SealImpressionEllipseEngineInitConfig, SealImpressionEngineRunConfig)
