"""The containers of the reference's font engine (vkit/engine/font/type.py:55-699): the run config and its style, the glyph
statistics ``build_char_glyph`` reads, ``CharBox``, ``CharGlyph`` and ``TextLine``.  Glyph rasterisation (freetype) stays outside
the package; the text-line half of the engine, which turns glyph bitmaps into a ``TextLine``, is ``text_line.py``.  ``TextLine``
has the fields of the page assembler's reduced text line (``image``, ``mask``, ``score_map``, ``glyph_color``, ``box``) and is
accepted wherever that one is.  The fields the seal-impression engine and the page assembler do not read are keyword fields with
defaults: a line or a glyph that came from elsewhere is built from the arrays alone."""
from enum import Enum, unique
from typing import Any, List, Mapping, Optional, Sequence, Tuple

import attrs
import numpy as np

from vkit_amd.element import Box, Image, Mask, Point, PointList, Polygon, ScoreMap, Shapable

_CV_INTER_CUBIC = 2


@attrs.define(frozen=True)
class FontGlyphInfo:
    tags: Sequence[str]
    ascent_plus_pad_up_min_to_font_size_ratio: float
    height_min_to_font_size_ratio: float
    width_min_to_font_size_ratio: float


@attrs.define
class FontGlyphInfoCollection:
    font_glyph_infos: Sequence[FontGlyphInfo]
    _tag_to_font_glyph_info: Optional[Mapping[str, FontGlyphInfo]] = attrs.field(default=None, init=False, repr=False, eq=False)

    @property
    def tag_to_font_glyph_info(self):
        if not self._tag_to_font_glyph_info:
            tag_to_font_glyph_info = {}
            for font_glyph_info in self.font_glyph_infos:
                assert font_glyph_info.tags
                for tag in font_glyph_info.tags:
                    assert tag not in tag_to_font_glyph_info
                    tag_to_font_glyph_info[tag] = font_glyph_info
            self._tag_to_font_glyph_info = tag_to_font_glyph_info
        return self._tag_to_font_glyph_info


@attrs.define
class FontVariant:
    char_to_tags: Mapping[str, Sequence[str]]
    font_file: Any
    font_glyph_info_collection: FontGlyphInfoCollection
    is_ttc: bool = False
    ttc_font_index: Optional[int] = None


@attrs.define
class FontEngineRunConfigStyle:
    # Font size.
    font_size_ratio: float = 1.0
    font_size_min: int = 12
    font_size_max: int = 96

    # Space between chars.
    prob_set_char_space_min: float = 0.5
    char_space_min: float = 0.0
    char_space_max: float = 0.2
    char_space_mean: float = 0.1
    char_space_std: float = 0.03

    # Space between words.
    word_space_min: float = 0.3
    word_space_max: float = 1.0
    word_space_mean: float = 0.6
    word_space_std: float = 0.1

    # Effect.
    glyph_color: Tuple[int, int, int] = (0, 0, 0)
    # https://en.wikipedia.org/wiki/Gamma_correction
    glyph_color_gamma: float = 1.0

    # Implementation related options.
    freetype_force_autohint: bool = False


@unique
class FontEngineRunConfigGlyphSequence(Enum):
    HORI_DEFAULT = 'hori_default'
    VERT_DEFAULT = 'vert_default'


@attrs.define
class FontEngineRunConfig:
    height: int
    width: int
    chars: Sequence[str]
    font_variant: FontVariant

    # Sequence mode.
    glyph_sequence: FontEngineRunConfigGlyphSequence = FontEngineRunConfigGlyphSequence.HORI_DEFAULT

    style: FontEngineRunConfigStyle = attrs.field(factory=FontEngineRunConfigStyle)

    # For debugging.
    return_font_variant: bool = False


@attrs.define(frozen=True)
class CharBox(Shapable):
    char: str
    box: Box

    def __attrs_post_init__(self):
        assert len(self.char) == 1 and not self.char.isspace()

    @property
    def up(self):
        return self.box.up

    @property
    def down(self):
        return self.box.down

    @property
    def left(self):
        return self.box.left

    @property
    def right(self):
        return self.box.right

    @property
    def height(self):
        return self.box.height

    @property
    def width(self):
        return self.box.width

    def to_conducted_resized_char_box(self, shapable_or_shape, resized_height: Optional[int] = None,
                                      resized_width: Optional[int] = None):
        return attrs.evolve(self, box=self.box.to_conducted_resized_box(shapable_or_shape=shapable_or_shape,
                                                                        resized_height=resized_height, resized_width=resized_width))

    def to_shifted_char_box(self, offset_y: int = 0, offset_x: int = 0):
        return attrs.evolve(self, box=self.box.to_shifted_box(offset_y=offset_y, offset_x=offset_x))


@attrs.define
class CharGlyph:
    image: Image
    score_map: Optional[ScoreMap]
    # the size of the font's reference char: what a char polygon is widened to
    ref_char_height: int
    ref_char_width: int
    # what build_char_glyph loads from the font face (reference :394-404)
    char: str = attrs.field(default='', kw_only=True)
    ascent: int = attrs.field(default=0, kw_only=True)
    pad_up: int = attrs.field(default=0, kw_only=True)
    pad_down: int = attrs.field(default=0, kw_only=True)
    pad_left: int = attrs.field(default=0, kw_only=True)
    pad_right: int = attrs.field(default=0, kw_only=True)
    ref_ascent_plus_pad_up: int = attrs.field(default=0, kw_only=True)

    def __attrs_post_init__(self):
        # NOTE: ascent could be negative for char like '_'.
        assert self.pad_up >= 0
        assert self.pad_down >= 0
        assert self.pad_left >= 0
        assert self.pad_right >= 0

    @property
    def height(self):
        return self.image.height

    @property
    def width(self):
        return self.image.width

    def get_glyph_mask(self, box: Optional[Box] = None, enable_resize: bool = False, cv_resize_interpolation: int = _CV_INTER_CUBIC):
        """``image > 0`` (any channel of an LCD glyph), resized to ``box`` if allowed and attached to it (reference :423-451)."""
        mat = self.image.mat
        if mat.ndim == 2:
            np_mask = mat > 0
        elif mat.ndim == 3:
            np_mask = np.any(mat > 0, axis=2)
        else:
            raise NotImplementedError()
        mask = Mask(mat=np_mask.astype(np.uint8))
        if box:
            if mask.shape != box.shape:
                assert enable_resize
                mask = mask.to_resized_mask(resized_height=box.height, resized_width=box.width,
                                            cv_resize_interpolation=cv_resize_interpolation)
            mask = mask.to_box_attached(box)
        return mask


@attrs.define
class TextLine:
    image: Image
    mask: Mask
    score_map: Optional[ScoreMap]
    char_boxes: Sequence[CharBox]
    # NOTE: char_glyphs might not have the same shapes as char_boxes.
    char_glyphs: Sequence[CharGlyph]
    cv_resize_interpolation: int
    is_hori: bool
    glyph_color: Tuple[int, int, int] = (0, 0, 0)
    # a shifted text line is bound to a page
    shifted: bool = False
    # what render_text_line_meta knows besides the arrays (reference :463-472); glyph_color is filled from style.glyph_color
    style: Optional[FontEngineRunConfigStyle] = attrs.field(default=None, kw_only=True)
    font_size: int = attrs.field(default=0, kw_only=True)
    text: str = attrs.field(default='', kw_only=True)
    # For debugging.
    font_variant: Optional[FontVariant] = attrs.field(default=None, kw_only=True)

    @property
    def box(self):
        assert self.mask.box
        return self.mask.box

    def to_shifted_text_line(self, offset_y: int = 0, offset_x: int = 0):
        self.shifted = True          # (the reference marks the line it was called on, :484)
        return attrs.evolve(
            self,
            image=self.image.to_shifted_image(offset_y=offset_y, offset_x=offset_x),
            mask=self.mask.to_shifted_mask(offset_y=offset_y, offset_x=offset_x),
            score_map=self.score_map.to_shifted_score_map(offset_y=offset_y, offset_x=offset_x) if self.score_map else None,
            char_boxes=[char_box.to_shifted_char_box(offset_y=offset_y, offset_x=offset_x) for char_box in self.char_boxes],
        )

    def to_polygon(self):
        """The outline of the line through the ends of its char boxes along the writing direction, with one point in the middle
        of each short side when the line is more than two pixels thick (reference :560-613)."""
        box = self.box
        if self.is_hori:
            begin, end, edges = box.left, box.right, [(char_box.left, char_box.right) for char_box in self.char_boxes]
        else:
            begin, end, edges = box.up, box.down, [(char_box.up, char_box.down) for char_box in self.char_boxes]
        stops = [begin]
        for lo, hi in edges:
            if stops[-1] < lo:
                stops.append(lo)
            if lo < hi:
                stops.append(hi)
        if stops[-1] < end:
            stops.append(end)
        points = PointList()
        if self.is_hori:
            mid = (box.up + box.down) // 2
            thick = box.up < mid < box.down
            points.extend(Point.create(y=box.up, x=x) for x in stops)
            if thick:
                points.append(Point.create(y=mid, x=stops[-1]))
            points.extend(Point.create(y=box.down, x=x) for x in reversed(stops))
            if thick:
                points.append(Point.create(y=mid, x=stops[0]))
        else:
            mid = (box.left + box.right) // 2
            thick = box.left < mid < box.right
            points.extend(Point.create(y=y, x=box.right) for y in stops)
            if thick:
                points.append(Point.create(y=stops[-1], x=mid))
            points.extend(Point.create(y=y, x=box.left) for y in reversed(stops))
            if thick:
                points.append(Point.create(y=stops[0], x=mid))
        return Polygon.create(points=points)

    def get_height_points(self, num_points: int, is_up: bool):
        """``num_points`` sample points along the up (a vertical line: right) or down (left) side (reference :701-732; a
        horizontal line samples x from 0, not from its left end, as the reference does)."""
        box = self.box
        if self.is_hori:
            stops = list(range(0, box.right + 1, max(1, box.width // num_points)))
            last = box.right
        else:
            stops = list(range(box.up, box.down + 1, max(1, box.height // num_points)))
            last = box.down
        if len(stops) >= num_points:
            stops = stops[:num_points - 1]
            stops.append(last)
        if self.is_hori:
            y = box.up if is_up else box.down
            return PointList(Point.create(y=y, x=x) for x in stops)
        x = box.right if is_up else box.left
        return PointList(Point.create(y=y, x=x) for y in stops)

    def get_char_level_height_points(self, is_up: bool):
        """One point a char at the middle of its box along the writing direction, on the up or down side (reference :734-755)."""
        box = self.box
        if self.is_hori:
            y = box.up if is_up else box.down
            return PointList(Point.create(y=y, x=(char_box.left + char_box.right) / 2) for char_box in self.char_boxes)
        x = box.right if is_up else box.left
        return PointList(Point.create(y=(char_box.up + char_box.down) / 2, x=x) for char_box in self.char_boxes)

    @classmethod
    def build_char_polygon(cls, up: float, down: float, left: float, right: float):
        return Polygon.from_xy_pairs([(left, up), (right, up), (right, down), (left, down)])

    def to_char_polygons(self, page_height: int, page_width: int, ref_char_height_ratio: float = 1.0,
                         ref_char_width_ratio: float = 1.0):
        """One rectangle a char, widened to the reference char's size inside the page (reference :630-699)."""
        assert len(self.char_boxes) == len(self.char_glyphs)
        polygons: List[Polygon] = []
        for char_box, char_glyph in zip(self.char_boxes, self.char_glyphs):
            ref_char_height = char_glyph.ref_char_height * ref_char_height_ratio
            ref_char_width = char_glyph.ref_char_width * ref_char_width_ratio
            box = char_box.box
            up, down, left, right = box.up, box.down, box.left, box.right
            if self.is_hori:
                if box.height < ref_char_height:
                    half_inc = (ref_char_height - box.height) / 2
                    up = max(0, up - half_inc)
                    down = min(page_height - 1, down + half_inc)
                if box.width < ref_char_width:
                    half_inc = (ref_char_width - box.width) / 2
                    left = max(0, left - half_inc)
                    right = min(page_width - 1, right + half_inc)
            else:
                if box.width < ref_char_height:
                    half_inc = (ref_char_height - box.width) / 2
                    left = max(0, left - half_inc)
                    right = min(page_width - 1, right + half_inc)
                if box.height < ref_char_width:
                    half_inc = (ref_char_width - box.height) / 2
                    up = max(self.box.up, up - half_inc)
                    down = min(page_height - 1, down + half_inc)
            polygons.append(self.build_char_polygon(up=up, down=down, left=left, right=right))
        return polygons
