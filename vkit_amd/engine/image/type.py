"""Run config of the image engines (reference: vkit/engine/image/type.py)."""
import attrs


@attrs.define
class ImageEngineRunConfig:
    height: int
    width: int
    disable_resizing: bool = False
