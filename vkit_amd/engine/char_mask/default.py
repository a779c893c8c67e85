"""The default char-mask engine: every char polygon filled into the mask, keep max (reference:
engine/char_mask/default.py:44-53) -- the ordered polygon paint of the label planes (csrc/polygon.hip)."""
from typing import Optional

import attrs
from numpy.random import Generator as RandomGenerator

from .type import CharMask, CharMaskEngineRunConfig


@attrs.define
class CharMaskDefaultEngineInitConfig:
    pass


class CharMaskDefaultEngine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'default'

    def __init__(self, init_config: Optional[CharMaskDefaultEngineInitConfig] = None, init_resource=None):
        self.init_config = init_config or CharMaskDefaultEngineInitConfig()

    def run(self, run_config: CharMaskEngineRunConfig, rng: Optional[RandomGenerator] = None) -> CharMask:
        from vkit_amd.pipeline.text_detection.page_distortion import paint_polygons
        mask, _ = paint_polygons((run_config.height, run_config.width), run_config.char_polygons)
        return CharMask(combined_chars_mask=mask)
