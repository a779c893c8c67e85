"""Barcode engines (reference: vkit/engine/barcode/): ``qr`` and ``code39``.  The encoders are third-party and injected
(``func_encode``); the module masks become score maps on the device, a page's worth in one call (``render_barcode_plans``)."""
from ..interface import EngineExecutorAggregatorFactory
from .type import BarcodeEngineRunConfig, BarcodePlan, render_barcode_plans
from .code39 import (
    barcode_code39_engine_executor_factory,
    BarcodeCode39EngineInitConfig,
    BarcodeCode39Engine,
)
from .qr import (
    barcode_qr_engine_executor_factory,
    BarcodeQrEngineInitConfig,
    BarcodeQrEngine,
)

barcode_engine_executor_aggregator_factory = EngineExecutorAggregatorFactory([
    barcode_code39_engine_executor_factory,
    barcode_qr_engine_executor_factory,
])

__all__ = [
    'BarcodeEngineRunConfig', 'BarcodePlan', 'render_barcode_plans', 'barcode_code39_engine_executor_factory',
    'BarcodeCode39EngineInitConfig', 'BarcodeCode39Engine', 'barcode_qr_engine_executor_factory', 'BarcodeQrEngineInitConfig',
    'BarcodeQrEngine', 'barcode_engine_executor_aggregator_factory',
]
