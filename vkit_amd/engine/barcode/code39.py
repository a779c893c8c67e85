"""The code-39 barcode engine (reference: vkit/engine/barcode/code39.py).  The encoder (python-barcode's ``Code39`` rendered by
the reference's ``NoTextImageWriter``) is third-party code and stays outside: ``func_encode(text) -> uint8 image`` (255
background, 0 ink) is injected, the default uses python-barcode and PIL when they import.  Everything after it is this
project's: the inverted mask, its trim to the ink with the reference's two asserts, the alpha draw, and on the device the score
map, its resize to the box and the clip (a SCORE record of ``vkx_page_layers_dev``)."""
import string
from typing import Callable, Optional

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd.element import ScoreMap
from ..interface import EngineExecutorFactory, NoneTypeEngineInitResource
from .type import BarcodeEngineRunConfig, BarcodePlan, render_barcode_plans


@attrs.define
class BarcodeCode39EngineInitConfig:
    aspect_ratio: float = 0.2854396602149411
    alpha_min: float = 0.7
    alpha_max: float = 1.0


def default_code39_encode(text: str) -> np.ndarray:
    try:
        from barcode import Code39
        from barcode.writer import BaseWriter, mm2px
        from PIL import Image as PilImage, ImageDraw as PilImageDraw
    except ImportError as exc:
        raise RuntimeError('the code-39 encoder needs python-barcode and PIL (pillow), which do not import here; '
                           'pass func_encode(text) -> uint8 image to BarcodeCode39Engine instead') from exc

    class NoTextImageWriter(BaseWriter):

        def __init__(self, mode: str = 'L'):
            super().__init__(self._init, self._paint_module, None, self._finish)
            self.mode = mode
            self.dpi = 300
            self._image = None
            self._draw = None

        def calculate_size(self, modules_per_line: int, number_of_lines: int):
            return 2 * self.quiet_zone + modules_per_line * self.module_width, 2.0 + self.module_height * number_of_lines

        def _init(self, code):
            width, height = self.calculate_size(len(code[0]), len(code))
            self._image = PilImage.new(self.mode, (int(mm2px(width, self.dpi)), int(mm2px(height, self.dpi))), self.background)
            self._draw = PilImageDraw.Draw(self._image)

        def _paint_module(self, xpos, ypos, width, color):
            size = [(mm2px(xpos, self.dpi), mm2px(ypos, self.dpi)),
                    (mm2px(xpos + width, self.dpi), mm2px(ypos + self.module_height, self.dpi))]
            self._draw.rectangle(size, outline=color, fill=color)

        def _finish(self):
            return self._image

    return np.asarray(Code39(code=text, writer=NoTextImageWriter()).render())


class BarcodeCode39Engine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'code39'

    @classmethod
    def convert_barcode_image_to_mask(cls, image: np.ndarray) -> np.ndarray:
        """The 0 / 1 ink mask of the encoder's image trimmed to its ink (reference: convert_barcode_pil_image_to_mask)."""
        mat = (~(np.asarray(image) > 0)).astype(np.uint8)

        # Trim.
        np_hori_nonzero = np.nonzero(np.amax(mat, axis=0))[0]
        assert len(np_hori_nonzero) >= 2
        left = int(np_hori_nonzero[0])
        right = int(np_hori_nonzero[-1])

        np_vert_nonzero = np.nonzero(np.amax(mat, axis=1))[0]
        assert len(np_vert_nonzero) >= 2
        up = int(np_vert_nonzero[0])
        down = int(np_vert_nonzero[-1])

        return np.ascontiguousarray(mat[up:down + 1, left:right + 1])

    def __init__(self, init_config: BarcodeCode39EngineInitConfig, init_resource: Optional[NoneTypeEngineInitResource] = None,
                 func_encode: Optional[Callable[[str], np.ndarray]] = None):
        self.init_config = init_config
        self.init_resource = init_resource
        self.ascii_letters = tuple(string.ascii_letters)
        self.func_encode = func_encode or default_code39_encode

    def plan(self, run_config: BarcodeEngineRunConfig, rng: Optional[RandomGenerator] = None) -> BarcodePlan:
        assert rng is not None
        num_chars = max(1, round(run_config.width / (run_config.height * self.init_config.aspect_ratio)))
        text = ''.join(rng.choice(self.ascii_letters) for _ in range(num_chars))
        mask = self.convert_barcode_image_to_mask(self.func_encode(text))
        alpha = float(rng.uniform(self.init_config.alpha_min, self.init_config.alpha_max))
        return BarcodePlan(mask=mask, alpha=alpha, height=run_config.height, width=run_config.width, text=text)

    def run(self, run_config: BarcodeEngineRunConfig, rng: Optional[RandomGenerator] = None) -> ScoreMap:
        return render_barcode_plans([self.plan(run_config, rng)])[0]


barcode_code39_engine_executor_factory = EngineExecutorFactory(BarcodeCode39Engine, BarcodeCode39EngineInitConfig,
                                                               BarcodeEngineRunConfig)
