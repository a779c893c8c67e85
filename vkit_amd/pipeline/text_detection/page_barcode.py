"""PageBarcodeStep (reference: vkit/pipeline/text_detection/page_barcode.py): the QR and code-39 score maps of a page.

``plan`` is the host half -- per box the engine's draws in the reference's order, QR boxes first -- and ``render`` makes the
score maps of ALL boxes in ONE ``vkx_page_layers_dev`` call (one launch).  Inside ``_native.resident(True)`` the maps are born
on the device and PageAssemblerStep composites them where they are.  The encoders are third-party and injected
(``func_encode_qr`` / ``func_encode_code39``, see ``vkit_amd.engine.barcode``)."""
from typing import Any, List, Mapping, Optional, Tuple

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd.element import Box
from vkit_amd.engine.barcode import (
    BarcodePlan,
    barcode_code39_engine_executor_factory,
    barcode_qr_engine_executor_factory,
    render_barcode_plans,
)
from ..interface import PipelineStep, PipelineStepFactory
from .page_assembler import PageBarcodeStepOutput, PageLayoutStepOutput


@attrs.define
class PageBarcodeStepConfig:
    barcode_qr_config: Optional[Mapping[str, Any]] = None
    barcode_code39_config: Optional[Mapping[str, Any]] = None


@attrs.define
class PageBarcodeStepInput:
    page_layout_step_output: PageLayoutStepOutput


@attrs.define
class PageBarcodePlan:
    height: int
    width: int
    qrs: List[Tuple[Box, BarcodePlan]]
    code39s: List[Tuple[Box, BarcodePlan]]


class PageBarcodeStep(PipelineStep[PageBarcodeStepConfig, PageBarcodeStepInput, PageBarcodeStepOutput]):

    def __init__(self, config: PageBarcodeStepConfig, func_encode_qr=None, func_encode_code39=None):
        super().__init__(config)
        self.barcode_qr_engine_executor = barcode_qr_engine_executor_factory.create(self.config.barcode_qr_config)
        self.barcode_code39_engine_executor = barcode_code39_engine_executor_factory.create(self.config.barcode_code39_config)
        if func_encode_qr is not None:
            self.barcode_qr_engine_executor.engine.func_encode = func_encode_qr
        if func_encode_code39 is not None:
            self.barcode_code39_engine_executor.engine.func_encode = func_encode_code39

    def plan(self, input: PageBarcodeStepInput, rng: RandomGenerator) -> PageBarcodePlan:
        page_layout = input.page_layout_step_output.page_layout
        qr_engine, code39_engine = self.barcode_qr_engine_executor.engine, self.barcode_code39_engine_executor.engine
        run_config_cls = self.barcode_qr_engine_executor.get_run_config_cls()

        qrs = []
        for layout_barcode_qr in page_layout.layout_barcode_qrs:
            box = layout_barcode_qr.box
            assert box.height == box.width
            qrs.append((box, qr_engine.plan(run_config_cls(height=box.height, width=box.width), rng)))

        code39s = []
        for layout_barcode_code39 in page_layout.layout_barcode_code39s:
            box = layout_barcode_code39.box
            code39s.append((box, code39_engine.plan(run_config_cls(height=box.height, width=box.width), rng)))

        return PageBarcodePlan(height=page_layout.height, width=page_layout.width, qrs=qrs, code39s=code39s)

    def render(self, plan: PageBarcodePlan) -> PageBarcodeStepOutput:
        pairs = plan.qrs + plan.code39s
        score_maps = render_barcode_plans([p for _, p in pairs], [box for box, _ in pairs])
        return PageBarcodeStepOutput(height=plan.height, width=plan.width, barcode_qr_score_maps=score_maps[:len(plan.qrs)],
                                     barcode_code39_score_maps=score_maps[len(plan.qrs):])

    def run(self, input: PageBarcodeStepInput, rng: RandomGenerator):
        return self.render(self.plan(input, rng))


page_barcode_step_factory = PipelineStepFactory(PageBarcodeStep)
