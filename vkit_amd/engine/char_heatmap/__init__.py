"""Char-heatmap engines (reference: vkit/engine/char_heatmap/): ``default``, the Gaussian char score map rasterised on the
device.  ``char_heatmap_default_engine_executor_factory.create(init_config)`` builds an executor whose ``run`` takes a
run config or the mapping of its fields."""
from .type import CharHeatmapEngineRunConfig, CharHeatmap
from .default import (
    build_np_distance,
    char_heatmap_default_engine_executor_factory,
    CharHeatmapDefaultDebug,
    CharHeatmapDefaultEngineInitConfig,
    CharHeatmapDefaultEngine,
)

__all__ = [
    'CharHeatmapEngineRunConfig', 'CharHeatmap', 'build_np_distance', 'char_heatmap_default_engine_executor_factory',
    'CharHeatmapDefaultDebug', 'CharHeatmapDefaultEngineInitConfig', 'CharHeatmapDefaultEngine',
]
