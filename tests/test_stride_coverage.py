"""CPU check: every strided export of include/vkx.h has a pitch-contract test or a stated exemption (tests/stride_table.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stride_table as T  # noqa: E402


def test_every_strided_export_is_tested_or_exempt():
    exports = set(T.strided_exports())
    assert 'vkx_resize_u8_dev' in exports and 'vkx_fill_u8_batch_dev' in exports      # the parser sees the header
    missing = sorted(exports - T.COVERED - set(T.EXEMPT))
    assert not missing, f'strided exports with neither a case in test_gpu_strides.py nor an exemption: {missing}'


def test_table_names_exist_and_do_not_overlap():
    exports = set(T.strided_exports())
    assert not (T.COVERED & set(T.EXEMPT)), sorted(T.COVERED & set(T.EXEMPT))
    stale = sorted((T.COVERED | set(T.EXEMPT)) - exports)
    assert not stale, f'names in tests/stride_table.py that vkx.h does not export with a stride: {stale}'
    assert all(reason.strip() for reason in T.EXEMPT.values())
    assert T.REFUSAL_TESTED <= exports, sorted(T.REFUSAL_TESTED - exports)


def test_struct_carried_strides_are_seen():
    """exports whose strides travel in a struct (element, layer, paint-set, noise-plane descriptors) count as strided"""
    exports = set(T.strided_exports())
    for name in ('vkx_remap_multi_dev', 'vkx_grid_remap_dev', 'vkx_paint_poly_sets_fresh_dev', 'vkx_noise_normal_i16_batch_dev',
                 'vkx_chain_rgb_batch_dev'):
        assert name in exports, name


def test_exemptions_are_down_to_host_wrappers_and_the_swap_lattice():
    assert {n for n, why in T.EXEMPT.items() if why != T._HOST_FORM} == {'vkx_glass_round_dev'}


def test_descriptor_fields_are_parsed_from_the_header():
    fields = T.struct_stride_fields()
    assert fields['vkx_chain_item'] == ['src_stride', 'dst_stride', 'noise_stride_el']
    assert fields['vkx_elem'] == ['src_stride', 'dst_stride'] and fields['vkx_noise_plane'] == ['stride_el']
    assert fields['vkx_paint_set'] == ['mask_stride', 'score_stride_el']
    assert set(fields['vkx_layer']) == {'mask_stride', 'alpha_stride_el', 'value_stride'}
    params = T.struct_params()
    assert params['vkx_chain_rgb_batch_np_dev'] == {'vkx_chain_item'} and params['vkx_fill_u8_dev_host_layers'] == {'vkx_layer'}
    assert all((name in T.COVERED) and struct in params[name] and field in fields[struct] and why.strip()
               for (name, struct, field), why in T.UNLAID_FIELDS.items())


def test_descriptor_cases_lay_out_every_strided_field():
    """a covered entry point whose strides travel in a struct has a descriptor case naming every strided field of the struct on
    a plane that takes the layouts (building the table of test_gpu_strides.py loads no library); a case that leaves a field
    out does not count"""
    import test_gpu_strides as S
    assert not T.descriptor_gaps(S.cases().values())

    class Partial:
        entry, dev_name, host, groups = 'vkx_remap_multi', 'vkx_remap_multi_dev', False, [('a',), ('b',)]
        descriptors = {'vkx_elem': [{'src_stride': 'a', 'dst_stride': 'elsewhere'}]}
    only = [c for c in S.cases().values() if c.dev_name != 'vkx_remap_multi_dev'] + [Partial]
    assert any('vkx_remap_multi_dev' in g and 'dst_stride' in g for g in T.descriptor_gaps(only))
