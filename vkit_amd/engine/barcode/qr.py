"""The QR barcode engine (reference: vkit/engine/barcode/qr.py).  The encoder (``cv.QRCodeEncoder``) is third-party code and
stays outside: ``func_encode(text) -> uint8 image`` (255 background, 0 ink) is injected, the default uses cv2 when it imports.
Everything after it is this project's: the inverted module mask, the alpha draw, and on the device the score map, its resize
to the box and the clip (a SCORE record of ``vkx_page_layers_dev``)."""
import string
from typing import Callable, Optional

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd.element import ScoreMap
from vkit_amd.utility import rng_choice_with_size
from ..interface import EngineExecutorFactory, NoneTypeEngineInitResource
from .type import BarcodeEngineRunConfig, BarcodePlan, render_barcode_plans

CV_PAYLOAD_TEXT_LENGTH_MAX = 150


@attrs.define
class BarcodeQrEngineInitConfig:
    payload_text_length_min: int = 1
    payload_text_length_max: int = CV_PAYLOAD_TEXT_LENGTH_MAX
    alpha_min: float = 0.7
    alpha_max: float = 1.0


def default_qr_encode(text: str) -> np.ndarray:
    try:
        import cv2 as cv
    except ImportError as exc:
        raise RuntimeError('the QR encoder needs cv2 (opencv-python), which does not import here; '
                           'pass func_encode(text) -> uint8 image to BarcodeQrEngine instead') from exc
    return cv.QRCodeEncoder.create().encode(text)


class BarcodeQrEngine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'qr'

    def __init__(self, init_config: BarcodeQrEngineInitConfig, init_resource: Optional[NoneTypeEngineInitResource] = None,
                 func_encode: Optional[Callable[[str], np.ndarray]] = None):
        self.init_config = init_config
        self.init_resource = init_resource
        assert self.init_config.payload_text_length_max <= CV_PAYLOAD_TEXT_LENGTH_MAX
        self.ascii_letters = tuple(string.ascii_letters)
        self.func_encode = func_encode or default_qr_encode

    def plan(self, run_config: BarcodeEngineRunConfig, rng: Optional[RandomGenerator] = None) -> BarcodePlan:
        assert rng is not None
        payload_text_length = rng.integers(self.init_config.payload_text_length_min, self.init_config.payload_text_length_max + 1)
        payload_text = ''.join(rng_choice_with_size(rng, self.ascii_letters, size=payload_text_length))
        # Black as activated pixels: Mask(mat=image).to_inverted_mask()
        image = np.asarray(self.func_encode(payload_text))
        mask = (~(image > 0)).astype(np.uint8)
        assert mask.ndim == 2 and mask.shape[0] == mask.shape[1]
        alpha = float(rng.uniform(self.init_config.alpha_min, self.init_config.alpha_max))
        return BarcodePlan(mask=mask, alpha=alpha, height=run_config.height, width=run_config.width, text=payload_text)

    def run(self, run_config: BarcodeEngineRunConfig, rng: Optional[RandomGenerator] = None) -> ScoreMap:
        return render_barcode_plans([self.plan(run_config, rng)])[0]


barcode_qr_engine_executor_factory = EngineExecutorFactory(BarcodeQrEngine, BarcodeQrEngineInitConfig, BarcodeEngineRunConfig)
