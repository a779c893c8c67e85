"""Char-mask engines (reference: vkit/engine/char_mask/): ``default`` (the polygon paint) and ``external_ellipse`` (discs
rasterised on the device).  ``char_mask_engine_executor_aggregator_factory.create_engine_executor({'type': ..., 'config':
{...}})`` builds one from the reference's config form."""
from typing import Any, Mapping, Optional, Union

import attrs

from .type import CharMaskEngineRunConfig, CharMask
from .default import CharMaskDefaultEngineInitConfig, CharMaskDefaultEngine
from .external_ellipse import CharMaskExternalEllipseEngineInitConfig, CharMaskExternalEllipseEngine


class CharMaskEngineExecutor:
    """``run`` takes a CharMaskEngineRunConfig or the mapping of its fields, as the reference's EngineExecutor does."""

    def __init__(self, engine):
        self.engine = engine

    def run(self, run_config: Union[CharMaskEngineRunConfig, Mapping[str, Any]], rng=None) -> CharMask:
        if not isinstance(run_config, CharMaskEngineRunConfig):
            run_config = CharMaskEngineRunConfig(**run_config)
        return self.engine.run(run_config, rng)


class CharMaskEngineExecutorAggregatorFactory:
    """The slice of the reference's EngineExecutorAggregatorFactory (engine/interface.py:279-411) the char-mask engines use."""

    def __init__(self, engine_classes):
        self.engine_classes = {cls.get_type_name(): (cls, init_cls) for cls, init_cls in engine_classes}

    def create_engine_executor(self, factory_init_config: Mapping[str, Any], init_resource: Optional[Any] = None):
        engine_type = factory_init_config.get('type')
        if engine_type not in self.engine_classes:
            raise NotImplementedError(f'char mask engine "{engine_type}" is outside the accelerated path')
        engine_cls, init_cls = self.engine_classes[engine_type]
        config = factory_init_config.get('config') or {}
        init_config = config if attrs.has(config.__class__) else init_cls(**dict(config))
        return CharMaskEngineExecutor(engine_cls(init_config, init_resource))


char_mask_engine_executor_aggregator_factory = CharMaskEngineExecutorAggregatorFactory([
    (CharMaskDefaultEngine, CharMaskDefaultEngineInitConfig),
    (CharMaskExternalEllipseEngine, CharMaskExternalEllipseEngineInitConfig),
])

__all__ = [
    'CharMaskEngineRunConfig', 'CharMask', 'CharMaskDefaultEngineInitConfig', 'CharMaskDefaultEngine',
    'CharMaskExternalEllipseEngineInitConfig', 'CharMaskExternalEllipseEngine', 'CharMaskEngineExecutor',
    'char_mask_engine_executor_aggregator_factory',
]
