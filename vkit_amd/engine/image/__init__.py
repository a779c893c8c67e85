"""Image engines (reference: vkit/engine/image/): ``combiner`` (a mosaic of texture tiles, built on the device) and
``selector`` (one file, a window of it or the file resized).  ``image_engine_executor_aggregator_factory.create([{'type': ...,
'weight': ..., 'config': {...}}, ...])`` builds the weighted list PageBackgroundStep draws from."""
from ..interface import EngineExecutorAggregatorFactory
from .type import ImageEngineRunConfig
from .combiner import (
    ImageMeta,
    load_image_metas_from_folder,
    ImageCombinerEngineInitConfig,
    ImageCombinerEngine,
    image_combiner_engine_executor_factory,
    plan_tiles,
)
from .selector import (
    ImageSelectorEngineInitConfig,
    ImageSelectorEngine,
    image_selector_engine_executor_factory,
)

image_engine_executor_aggregator_factory = EngineExecutorAggregatorFactory([
    image_combiner_engine_executor_factory,
    image_selector_engine_executor_factory,
])

__all__ = [
    'ImageEngineRunConfig', 'ImageMeta', 'load_image_metas_from_folder', 'ImageCombinerEngineInitConfig', 'ImageCombinerEngine',
    'image_combiner_engine_executor_factory', 'plan_tiles', 'ImageSelectorEngineInitConfig', 'ImageSelectorEngine',
    'image_selector_engine_executor_factory', 'image_engine_executor_aggregator_factory',
]
