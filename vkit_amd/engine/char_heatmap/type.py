"""Run config and result of the char-heatmap engines (reference: engine/char_heatmap/type.py)."""
from typing import Any, Sequence

import attrs

from vkit_amd.element import Polygon, ScoreMap


@attrs.define
class CharHeatmapEngineRunConfig:
    height: int
    width: int
    char_polygons: Sequence[Polygon]
    enable_debug: bool = False


@attrs.define
class CharHeatmap:
    score_map: ScoreMap
    debug: Any = None
