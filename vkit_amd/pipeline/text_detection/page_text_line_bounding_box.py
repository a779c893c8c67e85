"""PageTextLineBoundingBoxStep (reference: vkit/pipeline/text_detection/page_text_line_bounding_box.py): a frame around some
of a page's text lines.

``plan`` makes every draw in the reference's order (one ``rng.random()`` a line; for a framed line four offsets, the thickness,
the alpha) and every box decision (Python ``round``: half to even; the trims; both asserts); ``render`` makes ALL frames of the
page in ONE ``vkx_page_layers_dev`` call (one launch).  Inside ``_native.resident(True)`` the frames are born on the device."""
from typing import List, Tuple

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Box, ScoreMap
from vkit_amd.engine.page_layers import LayerBatch
from ..interface import PipelineStep, PipelineStepFactory
from .page_assembler import PageTextLineBoundingBoxStepOutput, PageTextLineStepOutput


@attrs.define
class PageTextLineBoundingBoxStepConfig:
    prob_non_short_text_line: float = 0.05
    prob_short_text_line: float = 0.3
    offset_ratio_min: float = 0.1
    offset_ratio_max: float = 2.0
    border_thickness_ratio_min: float = 0.0
    border_thickness_ratio_max: float = 0.125
    border_thickness_min: int = 1
    alpha_min: float = 0.9
    alpha_max: float = 1.0


@attrs.define
class PageTextLineBoundingBoxStepInput:
    page_text_line_step_output: PageTextLineStepOutput


@attrs.define
class TextLineBoundingBoxPlan:
    box_height: int
    box_width: int
    border_thickness: int
    alpha: float
    trims: Tuple[int, int, int, int]            # up, down, left, right
    page_box: Box
    color: Tuple[int, int, int]


class PageTextLineBoundingBoxStep(
        PipelineStep[PageTextLineBoundingBoxStepConfig, PageTextLineBoundingBoxStepInput, PageTextLineBoundingBoxStepOutput]):

    def sample_offset(self, ref_char_height: int, rng: RandomGenerator):
        offset_ratio = rng.uniform(self.config.offset_ratio_min, self.config.offset_ratio_max)
        return round(offset_ratio * ref_char_height)

    def sample_border_thickness(self, ref_char_height: int, rng: RandomGenerator):
        offset_ratio = rng.uniform(self.config.border_thickness_ratio_min, self.config.border_thickness_ratio_max)
        return max(round(offset_ratio * ref_char_height), self.config.border_thickness_min)

    def plan_text_line_bounding_box(self, height: int, width: int, text_line, rng: RandomGenerator) -> TextLineBoundingBoxPlan:
        ref_char_height_max = max(char_glyph.ref_char_height for char_glyph in text_line.char_glyphs)

        # Sample shape.
        offset_up = self.sample_offset(ref_char_height_max, rng)
        offset_down = self.sample_offset(ref_char_height_max, rng)
        offset_left = self.sample_offset(ref_char_height_max, rng)
        offset_right = self.sample_offset(ref_char_height_max, rng)

        box_height = text_line.box.height + offset_up + offset_down
        box_width = text_line.box.width + offset_left + offset_right

        border_thickness = self.sample_border_thickness(ref_char_height_max, rng)
        # (the reference draws uniform(alpha_max, alpha_max): the draw is consumed, the value is alpha_max)
        alpha = float(rng.uniform(self.config.alpha_max, self.config.alpha_max))

        empty_box = Box(up=border_thickness, down=box_height - border_thickness - 1, left=border_thickness,
                        right=box_width - border_thickness - 1)
        assert empty_box.up < empty_box.down
        assert empty_box.left < empty_box.right

        # Trim if out-of-boundary.
        page_box_up = text_line.box.up - offset_up
        page_box_down = text_line.box.down + offset_down
        page_box_left = text_line.box.left - offset_left
        page_box_right = text_line.box.right + offset_right

        trim_up_size = abs(page_box_up) if page_box_up < 0 else 0
        trim_down_size = page_box_down - height + 1 if page_box_down >= height else 0
        trim_left_size = abs(page_box_left) if page_box_left < 0 else 0
        trim_right_size = page_box_right - width + 1 if page_box_right >= width else 0

        page_box = Box(up=max(0, page_box_up), down=min(height - 1, page_box_down), left=max(0, page_box_left),
                       right=min(width - 1, page_box_right))
        return TextLineBoundingBoxPlan(box_height=box_height, box_width=box_width, border_thickness=border_thickness, alpha=alpha,
                                       trims=(trim_up_size, trim_down_size, trim_left_size, trim_right_size), page_box=page_box,
                                       color=text_line.glyph_color)

    def render_plans(self, plans: List[TextLineBoundingBoxPlan]) -> List[ScoreMap]:
        batch = LayerBatch()
        for plan in plans:
            batch.add_frame((plan.box_height, plan.box_width), plan.border_thickness, plan.alpha, plan.trims)
        resident = _native.resident_mode()
        return [ScoreMap.from_unchecked_mat(plane, box=plan.page_box) if resident else ScoreMap(mat=plane, box=plan.page_box)
                for plan, (_, plane) in zip(plans, batch.render(resident=resident))]

    def sample_text_line_bounding_box(self, height: int, width: int, text_line, rng: RandomGenerator):
        plan = self.plan_text_line_bounding_box(height, width, text_line, rng)
        return self.render_plans([plan])[0], plan.color

    def plan(self, input: PageTextLineBoundingBoxStepInput, rng: RandomGenerator) -> List[TextLineBoundingBoxPlan]:
        page_text_line_collection = input.page_text_line_step_output.page_text_line_collection
        plans = []
        for text_line, is_short_text_line in zip(page_text_line_collection.text_lines,
                                                 page_text_line_collection.short_text_line_flags):
            prob = self.config.prob_short_text_line if is_short_text_line else self.config.prob_non_short_text_line
            if not rng.random() < prob:
                continue
            plans.append(self.plan_text_line_bounding_box(page_text_line_collection.height, page_text_line_collection.width,
                                                          text_line, rng))
        return plans

    def render(self, plans: List[TextLineBoundingBoxPlan]) -> PageTextLineBoundingBoxStepOutput:
        return PageTextLineBoundingBoxStepOutput(score_maps=self.render_plans(plans), colors=[plan.color for plan in plans])

    def run(self, input: PageTextLineBoundingBoxStepInput, rng: RandomGenerator):
        return self.render(self.plan(input, rng))


page_text_line_bounding_box_step_factory = PipelineStepFactory(PageTextLineBoundingBoxStep)
