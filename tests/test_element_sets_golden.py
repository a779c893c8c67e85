"""CPU checks of the element set operations: the numpy restatement (tests/element_sets_restate.py) equals what the reference's
own Mask.from_* and fill_by_* produced (tests/golden/element_sets.npz, written by tests/golden/make_element_sets_golden.py),
bit for bit, and vkit_amd's uniqueness check decides as the reference's did."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import element_sets_restate as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'element_sets.npz')


@pytest.fixture(scope='module')
def golden():
    data = np.load(GOLDEN)
    index = json.loads(str(data['index']))

    def get(ref):
        at, shape, dtype = ref
        return data[dtype][at:at + int(np.prod(shape))].reshape(shape)
    return index, get


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_elements(kind, elements, stored, get):
    assert len(elements) == len(stored)
    for element, ref in zip(elements, stored):
        if kind == R.BOXES:
            assert list(element) == ref
        elif kind == R.POLYGONS:
            assert element.tolist() == get(ref).tolist()
        else:
            assert (bits(element[0]) == bits(get(ref['mat']))).all() and (element[1] and list(element[1])) == ref['box']


def test_the_fixture_is_small_and_data_only(golden):
    index, get = golden
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert len(index['from_cases']) == len(R.from_cases()) == 28 and len(index['fill_cases']) == len(R.fill_cases()) == 82
    for entry in index['from_cases'] + index['fill_cases']:
        assert max(entry['out'][1][:2]) <= 64


def test_constructor_cases_equal_the_reference(golden):
    index, get = golden
    for case, entry in zip(R.from_cases(), index['from_cases']):
        assert case['name'] == entry['name']
        same_elements(case['kind'], case['elements'], entry['elements'], get)
        want = get(entry['out'])
        got = R.restate_from(case)
        assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all(), case['name']
        assert entry['box'] == (case['attached'] and list(case['attached']))
        if case['elements'] and 'box' not in case['name']:
            assert want.any(), case['name']
    # the modes differ on these lists: a fixture of equal masks would pin nothing
    by_name = {e['name']: get(e['out']) for e in index['from_cases']}
    for kind in (R.BOXES, R.POLYGONS, R.MASKS, R.SCORE_MAPS):
        union, distinct, intersect = (by_name[f'from_{kind}_{mode}'] for mode in R.MODES)
        assert intersect.any() and distinct.any() and union.any()
        if kind in (R.BOXES, R.POLYGONS):      # (the planes of the other two kinds are drawn per case)
            assert ((distinct + intersect) == union).all()
        assert not by_name[f'from_{kind}_empty'].any()


def test_fill_cases_equal_the_reference(golden):
    index, get = golden
    changed = 0
    for case, entry in zip(R.fill_cases(), index['fill_cases']):
        assert case['name'] == entry['name']
        assert (bits(case['plane']) == bits(get(entry['plane']))).all()
        same_elements(case['kind'], case['elements'], entry['elements'], get)
        want = get(entry['out'])
        got = R.restate_fill(case)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert (bits(got) == bits(want)).all(), (case['name'], int((bits(got) != bits(want)).sum()))
        if case['elements']:
            changed += bool((bits(want) != bits(case['plane'])).any())
        else:
            assert (bits(want) == bits(case['plane'])).all()
    assert changed >= 70


def test_the_notch_triangle_is_filled_through_the_bounding_box_of_the_concave_polygon(golden):
    """the reference selects the set mask by a polygon's bounding box: the first polygon's value lands on pixels that belong
    only to the triangle in its notch"""
    case = next(c for c in R.fill_cases() if c['name'] == 'fill_image3_polygons_distinct_mixed')
    triangle = R.own_raster(R.POLYGONS, case['elements'][-1], R.SHAPE)
    concave = R.own_raster(R.POLYGONS, case['elements'][0], R.SHAPE)
    (up, down, left, right), raster = triangle
    inside_bbox = concave[0][0] <= up and down <= concave[0][1] and concave[0][2] <= left and right <= concave[0][3]
    assert inside_bbox and not concave[1][up - concave[0][0]:down + 1 - concave[0][0], left - concave[0][2]:right + 1 - concave[0][2]][raster].any()


def test_uniqueness_decisions(golden):
    import vkit_amd.element as E
    from vkit_amd.element.uniqueness import check_element_uniqueness, check_elements_uniqueness
    index, _ = golden
    seen = set()
    for case, entry in zip(R.fill_cases(), index['fill_cases']):
        if case['unique']:
            assert entry['unique'] is None
            continue
        values = [R.build_value(E, case, spec) for spec in case['values']]
        got = bool(check_elements_uniqueness(values))
        if case['dest'].startswith('image') and case['kind'] != R.SCORE_MAPS:
            shape = case['plane'].shape[:2]
            alphas = [R.alpha_of(case, i, R.box_of(case['kind'], raw, shape), False) for i, raw in enumerate(case['elements'])]
            got = bool(E.Image.check_values_and_alphas_uniqueness(values, alphas))
        assert got == entry['unique'] == R.restate_unique(case), case['name']
        seen.add(got)
    assert False in seen
    # the decisions the cases do not reach, by the rules of the reference (types first, then shape, then content; floats isclose)
    a = np.arange(6, dtype=np.uint8).reshape(2, 3)
    assert check_elements_uniqueness([]) and check_elements_uniqueness([3]) and check_elements_uniqueness([3, 3, 3])
    assert not check_elements_uniqueness([3, 3, 4]) and not check_element_uniqueness(3, 3.0)
    assert check_element_uniqueness(0.1 + 0.2, 0.3) and not check_element_uniqueness(0.3, 0.31)
    assert check_element_uniqueness((1, 2), (1, 2)) and not check_element_uniqueness((1, 2), (1, 3))
    assert check_element_uniqueness(a, a.copy()) and not check_element_uniqueness(a, a.astype(np.int32))
    assert not check_element_uniqueness(a, a.reshape(3, 2)) and not check_element_uniqueness(a, a + 1)
    f = np.array([0.1 + 0.2], np.float64)
    assert check_element_uniqueness(f, np.array([0.3])) and not check_element_uniqueness(f, np.array([0.4]))
    assert check_element_uniqueness(E.Mask(mat=a.copy()), E.Mask(mat=a.copy())) and not check_element_uniqueness(E.Mask(mat=a.copy()), a)
    s = np.full((2, 2), 0.3, np.float32)
    assert check_element_uniqueness(E.ScoreMap(mat=s.copy()), E.ScoreMap(mat=s + np.float32(1e-9)))
    with pytest.raises(NotImplementedError):
        check_element_uniqueness('a', 'a')


def test_the_reference_names_resolve():
    import vkit_amd.element as E
    from vkit_amd.element import box, mask, polygon, score_map, uniqueness
    for name in ('from_polygons', 'from_masks', 'from_score_maps', 'fill_by_box_value_pairs', 'fill_by_boxes',
                 'fill_by_polygon_value_pairs', 'fill_by_polygons', 'unpack_element_value_pairs', '__getitem__', '__setitem__',
                 'extract_score_map'):
        assert hasattr(E.Mask, name), name
    for name in ('fill_by_box_value_pairs', 'fill_by_boxes', 'fill_by_polygon_value_pairs', 'fill_by_polygons',
                 'fill_by_mask_value_pairs', 'fill_by_masks', 'unpack_element_value_pairs', '__getitem__', '__setitem__'):
        assert hasattr(E.ScoreMap, name), name
    for plural, kind in R.SINGULAR.items():
        assert hasattr(E.Image, f'fill_by_{kind}_value_tuples') and hasattr(E.Image, f'fill_by_{plural}')
    assert hasattr(E.Image, 'unpack_element_value_tuples') and hasattr(E.Image, 'check_values_and_alphas_uniqueness')
    assert hasattr(E.Box, 'extract_score_map') and hasattr(E.Polygon, 'extract_score_map')
    assert E.MaskSetItemConfig().value == 1 and E.ScoreMapSetItemConfig().value == 1.0
    assert uniqueness.check_element_uniqueness and uniqueness.check_elements_uniqueness
    union = E.ElementSetOperationMode.UNION
    assert (box.generate_fill_by_boxes_mask(R.SHAPE, [], union) is None and polygon.generate_fill_by_polygons_mask(R.SHAPE, [], union) is None
            and mask.generate_fill_by_masks_mask(R.SHAPE, [], union) is None
            and score_map.generate_fill_by_score_maps_mask(R.SHAPE, [], union) is None)
    elements, values, alphas = E.Image.unpack_element_value_tuples([('a', 1), ('b', 2, 0.5)])
    assert (elements, values, alphas) == (['a', 'b'], [1, 2], [1.0, 0.5])


def test_the_binding_lists_the_new_exports():
    from vkit_amd import _native
    assert {'vkx_set_mask', 'vkx_set_mask_dev'} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.SET_ELEM_DTYPE.itemsize == 56 and _native.SET_ELEM_DTYPE.fields['plane'][1] == 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vkx.h')).read()
    start = header.index('typedef struct vkx_set_elem')
    block = header[start:header.index('size_t window_bytes);', header.index('int vkx_set_mask(', start))]
    assert 'plane_step' in block and 'dst_step' in block and 'stride' not in block and 'pitch' not in block
