"""Seal-impression engines (reference: vkit/engine/seal_impression/): the ``ellipse`` engine, whose border and icon are drawn on
the device, and ``fill_text_line_to_seal_impression``, whose every pixel is (``fill_text_lines_to_seal_impressions`` takes all
seals of a page in one call)."""
from ..interface import EngineExecutorAggregatorFactory
from .type import CharSlot, TextLineSlot, SealImpression, SealImpressionEngineRunConfig
from .ellipse import (
    seal_impression_ellipse_engine_executor_factory,
    SealImpressionEllipseEngineInitConfig,
    SealImpressionEllipseEngine,
)
from .text_line_slot_filler import fill_text_line_to_seal_impression, fill_text_lines_to_seal_impressions

seal_impression_engine_executor_aggregator_factory = EngineExecutorAggregatorFactory([
    seal_impression_ellipse_engine_executor_factory,
])

__all__ = [
    'CharSlot', 'TextLineSlot', 'SealImpression', 'SealImpressionEngineRunConfig', 'SealImpressionEllipseEngineInitConfig',
    'SealImpressionEllipseEngine', 'seal_impression_ellipse_engine_executor_factory', 'fill_text_line_to_seal_impression',
    'fill_text_lines_to_seal_impressions', 'seal_impression_engine_executor_aggregator_factory',
]
