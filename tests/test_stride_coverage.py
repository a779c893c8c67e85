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
