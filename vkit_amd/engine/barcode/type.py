"""Run config and plan of the barcode engines (reference: vkit/engine/barcode/type.py)."""
import attrs
import numpy as np

from vkit_amd import _native
from vkit_amd.element import ScoreMap
from ..page_layers import LayerBatch


@attrs.define
class BarcodeEngineRunConfig:
    height: int
    width: int


@attrs.define
class BarcodePlan:
    """The host half of one barcode: the 0 / 1 module mask the encoder's image gives, the alpha drawn for it and the box's shape.
    ``LayerBatch.add_score`` takes it as it is."""
    mask: np.ndarray
    alpha: float
    height: int
    width: int
    text: str


def render_barcode_plans(plans, boxes=None):
    """The score maps of ``plans`` in ONE ``vkx_page_layers_dev`` call (one launch), each attached to its box of ``boxes``: device
    maps inside ``_native.resident(True)``, host maps of the reference's type otherwise."""
    batch = LayerBatch()
    for plan in plans:
        batch.add_score(plan.mask, (plan.height, plan.width), plan.alpha)
    resident = _native.resident_mode()
    score_maps = []
    for k, (_, plane) in enumerate(batch.render(resident=resident)):
        box = boxes[k] if boxes is not None else None
        score_maps.append(ScoreMap.from_unchecked_mat(plane, box=box) if resident else ScoreMap(mat=plane, box=box))
    return score_maps
