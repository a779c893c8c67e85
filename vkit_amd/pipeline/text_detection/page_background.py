"""PageBackgroundStep (reference: vkit/pipeline/text_detection/page_background.py): the page's background, an image of the
image engines (``weight_image``) or a constant grey page (``weight_random_grayscale``).

Inside ``_native.resident(True)`` the background is born on the device -- the combiner's mosaic by its one launch, the grey
page by a device fill -- and PageAssemblerStep takes it where it is.  ``image_configs`` is the reference's list of ``{type,
weight, config}`` mappings, or the path of a JSON file holding that list."""
from enum import Enum, unique
from typing import Any, Mapping, Sequence, Union

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Image
from vkit_amd.engine.image import image_engine_executor_aggregator_factory
from vkit_amd.utility import PathType, normalize_to_probs, rng_choice
from ..interface import PipelineStep, PipelineStepFactory
from .page_assembler import PageBackgroundStepOutput


@attrs.define
class PageShapeStepOutput:
    height: int
    width: int


@attrs.define
class PageBackgroundStepConfig:
    image_configs: Union[Sequence[Mapping[str, Any]], PathType]
    weight_image: float = 0.8
    weight_random_grayscale: float = 0.2
    grayscale_min: int = 127
    grayscale_max: int = 255


@attrs.define
class PageBackgroundStepInput:
    page_shape_step_output: PageShapeStepOutput


@unique
class PageBackgroundStepKey(Enum):
    IMAGE = 'image'
    RANDOM_GRAYSCALE = 'random_grayscale'


class PageBackgroundStep(PipelineStep[PageBackgroundStepConfig, PageBackgroundStepInput, PageBackgroundStepOutput]):

    def __init__(self, config: PageBackgroundStepConfig):
        super().__init__(config)
        self.image_engine_executor_aggregator = image_engine_executor_aggregator_factory.create(self.config.image_configs)
        self.keys = [PageBackgroundStepKey.IMAGE, PageBackgroundStepKey.RANDOM_GRAYSCALE]
        self.probs = normalize_to_probs([self.config.weight_image, self.config.weight_random_grayscale])

    def run(self, input: PageBackgroundStepInput, rng: RandomGenerator):
        page_shape_step_output = input.page_shape_step_output
        height = page_shape_step_output.height
        width = page_shape_step_output.width

        key = rng_choice(rng, self.keys, probs=self.probs)
        if key == PageBackgroundStepKey.IMAGE:
            background_image = self.image_engine_executor_aggregator.run({'height': height, 'width': width}, rng)
        elif key == PageBackgroundStepKey.RANDOM_GRAYSCALE:
            grayscale_value = rng.integers(self.config.grayscale_min, self.config.grayscale_max + 1)
            if _native.resident_mode():
                assert 0 <= grayscale_value <= 255
                background_image = Image(mat=_native.dev_full((height, width, 3), int(grayscale_value)))
            else:
                background_image = Image.from_shape((height, width), num_channels=3, value=grayscale_value)
        else:
            raise NotImplementedError()
        return PageBackgroundStepOutput(background_image=background_image)


page_background_step_factory = PipelineStepFactory(PageBackgroundStep)
