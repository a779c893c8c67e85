"""Slots, result and run config of the seal-impression engines (reference: vkit/engine/seal_impression/type.py)."""
from typing import Optional, Sequence, Tuple

import attrs
import numpy as np

from vkit_amd.element import Box, Mask, Point


@attrs.define
class CharSlot:
    angle: int
    point_up: Point
    point_down: Point

    @classmethod
    def build(cls, point_up: Point, point_down: Point):
        """The slot whose angle is the direction from ``point_down`` to ``point_up`` in whole degrees of [0, 360]."""
        theta = np.arctan2(point_up.smooth_y - point_down.smooth_y, point_up.smooth_x - point_down.smooth_x)
        two_pi = 2 * np.pi
        theta = theta % two_pi
        return cls(angle=round(theta / two_pi * 360), point_up=point_up, point_down=point_down)


@attrs.define
class TextLineSlot:
    text_line_height: int
    char_aspect_ratio: float
    char_slots: Sequence[CharSlot]


@attrs.define
class SealImpression:
    alpha: float
    color: Tuple[int, int, int]
    background_mask: Mask
    text_line_slots: Sequence[TextLineSlot]
    internal_text_line_box: Optional[Box]

    @property
    def shape(self):
        return self.background_mask.shape


@attrs.define
class SealImpressionEngineRunConfig:
    height: int
    width: int
