"""The cases of the element set operations and their numpy restatement (tests/test_element_sets_golden.py checks it against
the reference's recorded outputs, tests/test_gpu_element_sets.py checks the GPU path against it).

A case is plain data -- shapes, integer tables, planes, value specs -- so that the same case can be built from the reference's
element classes (tests/golden/make_element_sets_golden.py), from vkit_amd's (``run_from`` / ``run_fill`` with the element
module as argument) and restated here over ``oracle.fill_poly`` (the raster) and ``oracle.fill`` (the blend):

  count plane      int32, + 1 under every list entry (an entry listed twice counts twice), then UNION > 0, DISTINCT == 1,
                   INTERSECT > 1.
  UNION fill       the entries in list order, each through its own selection (box: none; polygon: its raster; mask: > 0;
                   score map: itself as alpha).
  unique values    one fill of values[0] / alphas[0] (score maps: score_maps[0] as alpha) under the set mask.
  non-unique       per entry the window of the set mask over the entry's box (a polygon's BOUNDING box), for masks and score
                   maps ANDed with the entry's own active pixels -- and, as the reference drops the box of that window, filled
                   at the destination's ORIGIN instead of at the entry's box.
"""
import math

import numpy as np

import oracle as O

SHAPE = (40, 50)
MODES = ('union', 'distinct', 'intersect')
BOXES, POLYGONS, MASKS, SCORE_MAPS = 'boxes', 'polygons', 'masks', 'score_maps'
SINGULAR = {BOXES: 'box', POLYGONS: 'polygon', MASKS: 'mask', SCORE_MAPS: 'score_map'}

# (up, down, left, right): three overlapping pairwise and triply, two on the border, one 1 x 1, a duplicate of the first
BOX_LIST = [(5, 20, 5, 25), (10, 30, 15, 40), (15, 25, 20, 30), (30, 39, 40, 49), (0, 5, 0, 10), (35, 35, 3, 3), (5, 20, 5, 25)]
# (x, y): concave; horizontal edges and a repeated vertex; a one-pixel-wide sliver; two sharing an edge; the concave one again;
# one touching all four borders; a triangle in the notch of the concave one (inside its bounding box, outside its raster)
CONCAVE = [(5, 5), (30, 5), (30, 30), (18, 12), (5, 30)]
POLYGON_LIST = [CONCAVE, [(10, 8), (25, 8), (25, 8), (40, 20), (25, 20), (10, 20)], [(44, 2), (44, 30), (44, 37)],
                [(12, 22), (24, 22), (24, 36), (12, 36)], [(24, 22), (38, 22), (38, 36), (24, 36)], CONCAVE,
                [(0, 20), (25, 0), (49, 18), (22, 39)], [(15, 22), (21, 22), (18, 27)]]
NOTCH_PAIR = [CONCAVE, [(15, 22), (21, 22), (18, 27)]]
ATTACHED = (3, 36, 4, 45)        # shape_or_box given as a Box: the elements lie inside it


def blocky(rng, shape, cell=4, p=0.5):
    h, w = shape
    coarse = rng.random(((h + cell - 1) // cell, (w + cell - 1) // cell)) < p
    return np.kron(coarse, np.ones((cell, cell), bool))[:h, :w]


def plane_list(rng, shape, score, prob=False):
    """[(plane, box or None)]: two planes with an attached box, two of the full shape, the first one again."""
    h, w = shape
    out = []
    for box in ((4, 15, 6, 25), (10, 33, 18, 47), None, None):
        sub = shape if box is None else (box[1] - box[0] + 1, box[3] - box[2] + 1)
        active = blocky(rng, sub, 4, 0.45)
        if score:
            mat = rng.random(sub, dtype=np.float32)
            if not prob:
                mat = mat * 2 - 1                       # negatives: only > 0 counts
            mat[~active] = 0.0
            if not prob:
                mat[blocky(rng, sub, 2, 0.2)] = -0.25
        else:
            mat = active.astype(np.uint8) * np.uint8(rng.integers(1, 256))
        out.append((mat, box))
    out.append(out[0])
    return out


def quads(rng, shape, n):
    """n text-line-like quads (x, y) inside ``shape``."""
    h, w = shape
    out = []
    for _ in range(n):
        bw, bh = int(rng.integers(12, 60)), int(rng.integers(4, 14))
        x, y = int(rng.integers(0, w - bw)), int(rng.integers(4, h - bh - 4))
        dy = rng.integers(-3, 4, 4)
        out.append([(x, y + dy[0]), (x + bw, y + dy[1]), (x + bw, y + bh + dy[2]), (x, y + bh + dy[3])])
    return out


def elements_of(kind, rng, shape=SHAPE, prob=False):
    if kind == BOXES:
        return list(BOX_LIST)
    if kind == POLYGONS:
        return [np.array(p, np.int32) for p in POLYGON_LIST]
    return plane_list(rng, shape, kind == SCORE_MAPS, prob)


# ---- the Mask.from_* cases -----------------------------------------------------------------------------------------------
def from_cases():
    cases = []
    for kind in (BOXES, POLYGONS, MASKS, SCORE_MAPS):
        for mode in MODES:
            rng = np.random.default_rng([11, len(cases)])
            cases.append(dict(name=f'from_{kind}_{mode}', kind=kind, mode=mode, shape=SHAPE, attached=None,
                              elements=elements_of(kind, rng)))
            # relative to a Box: only the elements inside it
            inside = [e for e in elements_of(kind, rng) if _inside(kind, e, ATTACHED)]
            cases.append(dict(name=f'from_{kind}_{mode}_box', kind=kind, mode=mode, shape=None, attached=ATTACHED, elements=inside))
        cases.append(dict(name=f'from_{kind}_empty', kind=kind, mode='union', shape=SHAPE, attached=None, elements=[]))
    return cases


def _inside(kind, element, box):
    up, down, left, right = box
    if kind == BOXES:
        u, d, l, r = element
    elif kind == POLYGONS:
        l, u = element.min(axis=0)
        r, d = element.max(axis=0)
    elif element[1] is None:
        return False
    else:
        u, d, l, r = element[1]
    return up <= u and d <= down and left <= l and r <= right


def big_case(n=200, shape=(256, 256)):
    """the 200-polygon list of text-line-like quads (restatement only: too large for the fixture)"""
    rng = np.random.default_rng(2024)
    return [np.array(q, np.int32) for q in quads(rng, shape, n)], shape


# ---- the fill_by_* cases -------------------------------------------------------------------------------------------------
DESTS = {'image3': (BOXES, POLYGONS, MASKS, SCORE_MAPS), 'image1': (BOXES, POLYGONS, MASKS, SCORE_MAPS),
         'mask': (BOXES, POLYGONS), 'score_map': (BOXES, POLYGONS, MASKS)}


def dest_plane(dest, rng, shape=SHAPE):
    if dest == 'image3':
        return rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    if dest == 'image1':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dest == 'mask':
        return blocky(rng, shape, 5, 0.3).astype(np.uint8)
    return (rng.random(shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32)


def value_spec(dest, rng, form, shape=SHAPE):
    """('scalar' | 'tuple' | 'array' | 'element', payload): array and element values have the destination's full shape."""
    if form in ('array', 'element'):
        if dest == 'mask':
            return (form, blocky(rng, shape, 3, 0.6).astype(np.uint8))
        if dest == 'score_map':
            return (form, rng.random(shape, dtype=np.float32))
        return (form, rng.integers(0, 256, shape + ((3,) if dest == 'image3' else ()), dtype=np.uint8))
    if dest == 'mask':
        return ('scalar', int(rng.integers(0, 2)))
    if dest == 'score_map':
        return ('scalar', float(rng.random()))
    if form == 'tuple' and dest == 'image3':
        return ('tuple', tuple(int(v) for v in rng.integers(0, 256, 3)))
    return ('scalar', int(rng.integers(0, 256)))


def fill_cases():
    cases = []
    forms = ('scalar', 'tuple', 'array', 'element')
    for dest, kinds in DESTS.items():
        for kind in kinds:
            for mode in MODES:
                for unique in (True, False):
                    k = len(cases)
                    rng = np.random.default_rng([7, k])
                    prob = kind == SCORE_MAPS
                    elements = elements_of(kind, rng, prob=prob)
                    if kind == SCORE_MAPS:
                        # (score_maps[0] is the alpha of the one fill under the set mask: it has to cover the destination)
                        elements = elements[2:] + elements[:2]
                    if kind == POLYGONS and not unique and mode != 'union':
                        elements = elements + [np.array(NOTCH_PAIR[1], np.int32)]
                    n = len(elements)
                    form = forms[k % 4]
                    if unique:
                        values = [value_spec(dest, rng, form)] * n
                    else:
                        values = [value_spec(dest, rng, forms[(k + i) % 4]) for i in range(n)]
                    selection = kind != BOXES or mode != 'union'
                    alphas = None
                    if dest.startswith('image') and kind != SCORE_MAPS:
                        choice = ('one', 'half', 'plane')[k % 3]
                        if choice == 'half' and dest == 'image1' and selection:
                            choice = 'plane'       # (the reference cannot blend a scalar alpha under a selection on a 2-D array)
                        alphas = choice
                    keep = (None, 'max', 'min')[k % 3] if dest in ('mask', 'score_map') else None
                    cases.append(dict(name=f'fill_{dest}_{kind}_{mode}_{"unique" if unique else "mixed"}', dest=dest, kind=kind,
                                      mode=mode, unique=unique, elements=elements, values=values, alphas=alphas, keep=keep,
                                      plane=dest_plane(dest, rng), seed=k))
    # empty lists: a fill that changes nothing
    for dest in DESTS:
        rng = np.random.default_rng([9, len(cases)])
        cases.append(dict(name=f'fill_{dest}_empty', dest=dest, kind=BOXES, mode='union', unique=True, elements=[], values=[],
                          alphas=None, keep=None, plane=dest_plane(dest, rng), seed=len(cases)))
    return cases


def box_of(kind, element, shape):
    if kind == BOXES:
        return tuple(element)
    if kind == POLYGONS:
        left, up = element.min(axis=0)
        right, down = element.max(axis=0)
        return (int(up), int(down), int(left), int(right))
    return element[1] or (0, shape[0] - 1, 0, shape[1] - 1)


def alpha_of(case, index, box, full):
    """the alpha of entry ``index`` (``full``: over the whole destination, else over the entry's box): 1.0, 0.5 or a plane"""
    if case['alphas'] in (None, 'one'):
        return 1.0
    if case['alphas'] == 'half':
        return 0.5
    shape = case['plane'].shape[:2] if full else (box[1] - box[0] + 1, box[3] - box[2] + 1)
    rng = np.random.default_rng([13, case['seed'], 0 if case['unique'] else index])
    alpha = rng.random(shape, dtype=np.float32)
    alpha[blocky(rng, shape, 3, 0.3)] = 0.0
    return alpha


# ---- running a case through an element module (the reference's or vkit_amd's) ---------------------------------------------
def build_elements(E, kind, elements, on_device=None):
    """``on_device``: a callable host array -> device array for the element planes (vkit_amd only)."""
    put = on_device or (lambda a: a)
    out = []
    for element in elements:
        if kind == BOXES:
            out.append(E.Box(up=element[0], down=element[1], left=element[2], right=element[3]))
        elif kind == POLYGONS:
            out.append(E.Polygon.from_xy_pairs([(int(x), int(y)) for x, y in element]))
        else:
            mat, box = element
            box = box and E.Box(up=box[0], down=box[1], left=box[2], right=box[3])
            if kind == MASKS:
                out.append(E.Mask(mat=put(mat.copy()), box=box))
            else:
                prob = bool(mat.min() >= 0.0)
                out.append(E.ScoreMap(mat=put(mat.copy()), box=box, is_prob=prob))
    return out


def mode_of(E, mode):
    return E.ElementSetOperationMode(mode)


def run_from(E, case, on_device=None):
    """Mask.from_<kind> -> the Mask"""
    elements = build_elements(E, case['kind'], case['elements'], on_device)
    where = E.Box(up=case['attached'][0], down=case['attached'][1], left=case['attached'][2], right=case['attached'][3]) \
        if case['attached'] else case['shape']
    return getattr(E.Mask, f'from_{case["kind"]}')(where, elements, mode_of(E, case['mode']))


def build_dest(E, case, put=None):
    put = put or (lambda a: a)
    plane = put(case['plane'].copy())
    if case['dest'] == 'mask':
        return E.Mask(mat=plane)
    if case['dest'] == 'score_map':
        return E.ScoreMap(mat=plane)
    return E.Image(mat=plane)


def build_value(E, case, spec):
    form, payload = spec
    if form == 'element':
        cls = {'mask': E.Mask, 'score_map': E.ScoreMap}.get(case['dest'], E.Image)
        return cls(mat=payload.copy())
    return payload.copy() if form == 'array' else payload


def run_fill(E, case, put=None):
    """dest.fill_by_<kind>... -> the destination element, filled.  Unique cases go through the plural form (one value), mixed
    ones through the pairs / tuples form."""
    dest, kind = build_dest(E, case, put), case['kind']
    elements = build_elements(E, kind, case['elements'], put)
    mode = mode_of(E, case['mode'])
    shape = case['plane'].shape[:2]
    kwargs = {}
    if case['keep']:
        kwargs[f'keep_{case["keep"]}_value'] = True
    is_image = case['dest'].startswith('image')
    if case['unique'] and case['elements']:
        value = build_value(E, case, case['values'][0])
        full = case['mode'] != 'union'
        if is_image and kind != SCORE_MAPS:
            if full or case['alphas'] != 'plane':
                kwargs['alpha'] = alpha_of(case, 0, None, True)
                getattr(dest, f'fill_by_{kind}')(elements, value, mode=mode, **kwargs)
            else:       # a plane of every entry's own shape: the tuples form, check skipped as the plural form skips it
                tuples = [(e, value, alpha_of(case, i, box_of(kind, raw, shape), False))
                          for i, (e, raw) in enumerate(zip(elements, case['elements']))]
                getattr(dest, f'fill_by_{SINGULAR[kind]}_value_tuples')(tuples, mode=mode, skip_values_uniqueness_check=True)
        else:
            getattr(dest, f'fill_by_{kind}')(elements, value, mode=mode, **kwargs)
        return dest
    values = [build_value(E, case, spec) for spec in case['values']]
    if is_image:
        if kind == SCORE_MAPS:
            tuples = list(zip(elements, values))
        else:
            tuples = [(e, v, alpha_of(case, i, box_of(kind, raw, shape), False))
                      for i, (e, v, raw) in enumerate(zip(elements, values, case['elements']))]
        getattr(dest, f'fill_by_{SINGULAR[kind]}_value_tuples')(tuples, mode=mode)
    else:
        getattr(dest, f'fill_by_{SINGULAR[kind]}_value_pairs')(list(zip(elements, values)), mode=mode, **kwargs)
    return dest


# ---- the restatement -------------------------------------------------------------------------------------------------------
def own_raster(kind, element, shape):
    """(box, bool raster over the box) of one entry"""
    box = box_of(kind, element, shape)
    up, down, left, right = box
    if kind == BOXES:
        return box, np.ones((down - up + 1, right - left + 1), bool)
    if kind == POLYGONS:
        return box, O.fill_poly((down - up + 1, right - left + 1), element - np.array([left, up], np.int32)) > 0
    return box, element[0] > 0


def set_mask(kind, elements, shape, mode, origin=(0, 0)):
    count = np.zeros(shape, np.int32)
    for element in elements:
        (up, down, left, right), raster = own_raster(kind, element, (shape[0] + origin[0], shape[1] + origin[1]))
        count[up - origin[0]:down + 1 - origin[0], left - origin[1]:right + 1 - origin[1]][raster] += 1
    return {'union': count > 0, 'distinct': count == 1, 'intersect': count > 1}[mode].astype(np.uint8)


def restate_from(case):
    if case['attached']:
        up, down, left, right = case['attached']
        return set_mask(case['kind'], case['elements'], (down - up + 1, right - left + 1), case['mode'], (up, left))
    return set_mask(case['kind'], case['elements'], case['shape'], case['mode'])


def same_value(a, b):
    """check_element_uniqueness on two value specs"""
    if a[0] != b[0] or type(a[1]) is not type(b[1]):
        return False
    if isinstance(a[1], np.ndarray):
        if a[1].shape != b[1].shape or a[1].dtype != b[1].dtype:
            return False
        if np.issubdtype(a[1].dtype, np.floating):
            return bool(np.isclose(a[1], b[1]).all())
        return bool((a[1] == b[1]).all())
    if isinstance(a[1], float):
        return math.isclose(a[1], b[1])
    return a[1] == b[1]


def restate_unique(case):
    """the decision of check_elements_uniqueness over the values (and, for image destinations, the alphas) of a mixed case"""
    values = case['values']
    unique = all(same_value(values[0], v) for v in values[1:])
    if case['dest'].startswith('image') and case['kind'] != SCORE_MAPS and case['alphas'] == 'plane':
        shape = case['plane'].shape[:2]
        alphas = [alpha_of(case, i, box_of(case['kind'], raw, shape), False) for i, raw in enumerate(case['elements'])]
        unique = unique and all(a.shape == alphas[0].shape and bool(np.isclose(alphas[0], a).all()) for a in alphas[1:])
    return unique


def _blend(plane, box, spec, mask, alpha, keep):
    up, down, left, right = box
    value = spec[1]
    if isinstance(value, np.ndarray):
        value = np.ascontiguousarray(value[up:down + 1, left:right + 1]).astype(plane.dtype)
    mode = {None: O.FILL_PLAIN, 'max': O.FILL_KEEP_MAX, 'min': O.FILL_KEEP_MIN}[keep]
    O.fill(plane, (up, left, down - up + 1, right - left + 1), value, mask=None if mask is None else mask.astype(np.uint8),
           alpha=alpha, mode=mode)


def restate_fill(case):
    plane = case['plane'].copy()
    kind, elements, values, mode, keep = case['kind'], case['elements'], case['values'], case['mode'], case['keep']
    shape = plane.shape[:2]
    if not elements:
        return plane
    plural = case['unique']
    if mode == 'union':
        for i, (element, spec) in enumerate(zip(elements, values)):
            box, raster = own_raster(kind, element, shape)
            if kind == SCORE_MAPS:
                _blend(plane, box, spec, None, element[0], keep)
            else:
                _blend(plane, box, spec, None if kind == BOXES else raster, alpha_of(case, i, box, False), keep)
        return plane
    chosen = set_mask(kind, elements, shape, mode)
    full = (0, shape[0] - 1, 0, shape[1] - 1)
    if plural or restate_unique(case):
        alpha = elements[0][0] if kind == SCORE_MAPS else alpha_of(case, 0, full if plural else box_of(kind, elements[0], shape), plural)
        _blend(plane, full, values[0], chosen, alpha, keep)
        return plane
    for i, (element, spec) in enumerate(zip(elements, values)):
        box, raster = own_raster(kind, element, shape)
        window = chosen[box[0]:box[1] + 1, box[2]:box[3] + 1] > 0
        if kind in (MASKS, SCORE_MAPS):
            # the reference extracts this window without its box and fills through it as it is: at the destination's origin
            window = window & raster
            box = (0, box[1] - box[0], 0, box[3] - box[2])
        _blend(plane, box, spec, window, element[0] if kind == SCORE_MAPS else alpha_of(case, i, box, False), keep)
    return plane
