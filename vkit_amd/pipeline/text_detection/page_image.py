"""PageImageStep (reference: vkit/pipeline/text_detection/page_image.py): the images of a page and its bottom layer.

``plan`` and the render are one here: the image engines (``vkit_amd.engine.image``) make their own draws and build their
images on the device already; per layout image one aggregator run and one ``rng.uniform`` for alpha, then the bottom layer --
one run with ``disable_resizing``, ``rng_choice(rng, (0, 90, 180, 270))`` and ``rotate.distort_image``.  The step adds no
kernel."""
from typing import Any, List, Mapping, Sequence, Union

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd.engine.image import image_engine_executor_aggregator_factory
from vkit_amd.mechanism.distortion import rotate
from vkit_amd.utility import PathType, rng_choice
from ..interface import PipelineStep, PipelineStepFactory
from .page_assembler import PageImage, PageImageCollection, PageImageStepOutput, PageLayoutStepOutput


@attrs.define
class PageImageStepConfig:
    image_configs: Union[Sequence[Mapping[str, Any]], PathType]
    alpha_min: float = 0.25
    alpha_max: float = 1.0


@attrs.define
class PageImageStepInput:
    page_layout_step_output: PageLayoutStepOutput


class PageImageStep(PipelineStep[PageImageStepConfig, PageImageStepInput, PageImageStepOutput]):

    def __init__(self, config: PageImageStepConfig):
        super().__init__(config)
        self.image_engine_executor_aggregator = image_engine_executor_aggregator_factory.create(self.config.image_configs)

    def run(self, input: PageImageStepInput, rng: RandomGenerator):
        page_layout = input.page_layout_step_output.page_layout

        page_images: List[PageImage] = []
        for layout_image in page_layout.layout_images:
            image = self.image_engine_executor_aggregator.run(
                {'height': layout_image.box.height, 'width': layout_image.box.width}, rng)
            alpha = float(rng.uniform(self.config.alpha_min, self.config.alpha_max))
            page_images.append(PageImage(image=image, box=layout_image.box, alpha=alpha))

        page_image_collection = PageImageCollection(height=page_layout.height, width=page_layout.width, page_images=page_images)

        page_bottom_layer_image = self.image_engine_executor_aggregator.run(
            {'height': 0, 'width': 0, 'disable_resizing': True}, rng)
        # Random rotate.
        rotate_angle = rng_choice(rng, (0, 90, 180, 270))
        page_bottom_layer_image = rotate.distort_image({'angle': rotate_angle}, page_bottom_layer_image)

        return PageImageStepOutput(page_image_collection=page_image_collection, page_bottom_layer_image=page_bottom_layer_image)


page_image_step_factory = PipelineStepFactory(PageImageStep)
