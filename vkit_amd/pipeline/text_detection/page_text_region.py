"""The output of the reference's PageTextRegionStep (vkit/pipeline/text_detection/page_text_region.py:177-186), the input of
PageTextRegionLabelStep.  Data only: the step that produces it (shapely, STRtree, rectpack) is outside the accelerated path,
so its output enters here as a plain container, as the inputs of page_assembler.py do."""
from typing import Any, Optional, Sequence, Tuple

import attrs

from vkit_amd.element import Image, Mask, Polygon


@attrs.define
class PageTextRegionStepOutput:
    page_image: Image
    page_active_mask: Mask
    page_char_polygons: Sequence[Polygon]
    page_text_region_polygons: Sequence[Polygon]
    page_char_polygon_text_region_polygon_indices: Sequence[int]
    shape_before_rotate: Tuple[int, int]
    rotate_angle: int
    debug: Optional[Any]
