"""Do the values of a ``fill_by_*`` list all say the same?  (reference: vkit/element/uniqueness.py:20-83)

Decides between the two non-UNION paths of the ``fill_by_*`` families: one fill of the first value under the set mask, or one
fill an element.  Values of different types differ; planes are compared by shape and then by content, float content and float
scalars with numpy's / math's default ``isclose`` tolerances, as the reference compares them."""
import math

import numpy as np


def check_element_uniqueness(value0, value1):
    if type(value0) is not type(value1):
        return False
    if isinstance(value0, (Image, Mask)):
        return value0.shape == value1.shape and bool((value0.mat == value1.mat).all())
    if isinstance(value0, ScoreMap):
        return value0.shape == value1.shape and bool(np.isclose(value0.mat, value1.mat).all())
    if isinstance(value0, np.ndarray):
        if value0.shape != value1.shape or value0.dtype != value1.dtype:
            return False
        if np.issubdtype(value0.dtype, np.floating):
            return bool(np.isclose(value0, value1).all())
        return bool((value0 == value1).all())
    if isinstance(value0, tuple):
        assert len(value0) == len(value1)
        return value0 == value1
    if isinstance(value0, int):
        return value0 == value1
    if isinstance(value0, float):
        return math.isclose(value0, value1)
    raise NotImplementedError()


def check_elements_uniqueness(values):
    """Every value against the first one."""
    return all(check_element_uniqueness(values[0], value) for value in values[1:])


# Cyclic by design, like the reference.
from .mask import Mask  # noqa: E402
from .score_map import ScoreMap  # noqa: E402
from .image import Image  # noqa: E402
