"""The strided exports of include/vkx.h and where their pitch contract is tested.

Every exported function with a `stride` or `pitch` parameter, or with a parameter whose struct type carries a `*_stride`
field (vkx_elem, vkx_layer, vkx_paint_set, vkx_noise_plane, vkx_chain_item, ...), is either exercised by
tests/test_gpu_strides.py (COVERED: its cases run the entry point on offset, padded and windowed planes) or listed in EXEMPT
with the reason it is not.  tests/test_stride_coverage.py checks on the CPU that nothing falls between the two; the GPU module
checks that every name in COVERED has a case.  An exemption is from the layout cases only: the refusal of short and negative
strides is tested for every entry point named in REFUSAL_TESTED too.  Nothing here loads libvkx.so.

The chain (vkx_chain_item: fused and staged kernels, plane and tiled noise), the multi-element lattice and map remaps
(vkx_elem), the grid map, the polygon raster and paint family (vkx_paint_set), the batched noise planes (vkx_noise_plane) and
the composite with host layers (vkx_layer) are covered by descriptor cases: a case counts for its entry point only if it lays
out every strided field of the struct (descriptor_gaps), and each run checks that the descriptors carried those strides.
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vkx.h')

# device entry points with a case of their own in test_gpu_strides.py
COVERED_DEV = {
    'vkx_remap_u8_dev', 'vkx_remap_f32_dev',
    'vkx_warp_affine_u8_dev', 'vkx_warp_affine_f32_dev', 'vkx_warp_perspective_u8_dev', 'vkx_warp_perspective_f32_dev',
    'vkx_gaussian_blur_u8_dev', 'vkx_filter2d_u8_dev',
    'vkx_color_shift_rgb_dev', 'vkx_cvt_rgb_hsv_u8_dev', 'vkx_mean_shift_u8_dev', 'vkx_add_noise_i16_dev',
    'vkx_brightness_shift_rgb_dev', 'vkx_color_balance_rgb_dev', 'vkx_pointwise_u8_dev', 'vkx_apply_lut_u8_dev',
    'vkx_impulse_noise_u8_dev', 'vkx_histogram_u8_dev',
    'vkx_line_streak_u8_dev', 'vkx_ellipse_mask_u8_dev', 'vkx_ellipse_streak_u8_dev',
    'vkx_cvt_color_u8_dev', 'vkx_blend_u8_dev', 'vkx_fog_f32_u8_dev', 'vkx_sum_f32_u8_dev', 'vkx_gather_u8_dev',
    'vkx_speckle_noise_u8_dev', 'vkx_fill_u8_dev', 'vkx_fill_u8_batch_dev', 'vkx_fill_f32_dev',
    'vkx_resize_cubic_u8_dev', 'vkx_resize_cubic_f32_dev', 'vkx_resize_u8_dev', 'vkx_resize_f32_dev',
    'vkx_jpeg_roundtrip_u8_dev', 'vkx_zoom_in_blur_u8_dev', 'vkx_noise_normal_i16_dev',
    # descriptor-carried strides and the raster / paint family
    'vkx_chain_rgb_batch_dev', 'vkx_chain_rgb_batch_np_dev', 'vkx_grid_remap_dev', 'vkx_remap_multi_dev', 'vkx_grid_to_map_dev',
    'vkx_fill_poly_mask_u8_dev', 'vkx_paint_polys_dev', 'vkx_paint_polys_fresh_dev', 'vkx_paint_poly_sets_fresh_dev',
    'vkx_noise_normal_i16_batch_dev', 'vkx_fill_u8_dev_host_layers',
}

# host entry points run on pitched host buffers with canaries: the pitched gather and copy-out of HostStage
# (vkit_amd/csrc/vkx_host_stage.h), and the plane copies of the three host forms that stage by hand (vkx_ellipse_mask_u8,
# vkx_ellipse_streak_u8, vkx_sum_f32_u8)
COVERED_HOST = {
    'vkx_remap_u8', 'vkx_warp_affine_u8', 'vkx_gaussian_blur_u8', 'vkx_filter2d_u8', 'vkx_color_shift_rgb', 'vkx_blend_u8',
    'vkx_fill_u8', 'vkx_resize_u8', 'vkx_resize_f32', 'vkx_line_streak_u8', 'vkx_speckle_noise_u8', 'vkx_fog_f32_u8',
    'vkx_gather_u8', 'vkx_jpeg_roundtrip_u8', 'vkx_zoom_in_blur_u8', 'vkx_cvt_color_u8', 'vkx_noise_normal_i16',
    'vkx_ellipse_mask_u8', 'vkx_ellipse_streak_u8', 'vkx_sum_f32_u8',
    'vkx_grid_remap', 'vkx_remap_multi', 'vkx_grid_to_map', 'vkx_paint_polys', 'vkx_fill_poly_mask_u8',
}

_HOST_FORM = 'the host form is a vkx_host_run call (vkit_amd/csrc/vkx_host_stage.h): the HostStage gather / copy-out of the ' \
             'host entry points of COVERED_HOST around the _dev form this table covers'

EXEMPT = {
    'vkx_remap_f32': _HOST_FORM,
    'vkx_warp_affine_f32': _HOST_FORM,
    'vkx_warp_perspective_u8': _HOST_FORM,
    'vkx_warp_perspective_f32': _HOST_FORM,
    'vkx_cvt_rgb_hsv_u8': _HOST_FORM,
    'vkx_mean_shift_u8': _HOST_FORM,
    'vkx_add_noise_i16': _HOST_FORM,
    'vkx_brightness_shift_rgb': _HOST_FORM,
    'vkx_color_balance_rgb': _HOST_FORM,
    'vkx_pointwise_u8': _HOST_FORM,
    'vkx_histogram_u8': _HOST_FORM,
    'vkx_apply_lut_u8': _HOST_FORM,
    'vkx_impulse_noise_u8': _HOST_FORM,
    'vkx_fill_f32': _HOST_FORM,
    'vkx_resize_cubic_u8': _HOST_FORM,
    'vkx_resize_cubic_f32': _HOST_FORM,
    'vkx_glass_round_dev': '`pitch` is the spacing of the swap lattice, not a row pitch; the planes are dense',
}

COVERED = COVERED_DEV | COVERED_HOST

# entry points outside the table's own refusal test whose refusal of short and negative strides test_gpu_strides.py tests all the same
REFUSAL_TESTED = {
    'vkx_fill_poly_mask_u8_dev', 'vkx_fill_poly_mask_u8', 'vkx_paint_polys_dev', 'vkx_paint_polys', 'vkx_paint_polys_fresh_dev',
    'vkx_paint_poly_sets_fresh_dev', 'vkx_grid_to_map_dev', 'vkx_remap_multi_dev', 'vkx_grid_remap_dev',
    'vkx_chain_rgb_batch_dev', 'vkx_chain_rgb_batch_np_dev',
}

# strided descriptor fields an entry point never reads in the form its cases call it in
UNLAID_FIELDS = {
    ('vkx_chain_rgb_batch_np_dev', 'vkx_chain_item', 'noise_stride_el'):
        'the noise of its items is the tile buffer of a stream job, which has no pitch (noise_tiled); a plane noise takes the '
        'code of vkx_chain_rgb_batch_dev, whose cases lay it out',
}


def strided_structs(text):
    """The struct types of vkx.h with a field whose name contains `stride`."""
    return {m.group(2) for m in re.finditer(r'typedef\s+struct\s+\w+\s*\{([^}]*)\}\s*(\w+)\s*;', text, flags=re.S)
            if 'stride' in m.group(1)}


def strided_exports(path=HEADER):
    """Names of the functions declared in vkx.h with a parameter whose name contains `stride` or `pitch`, or whose type is
    (a pointer to) a struct with a stride field."""
    with open(path) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    structs = strided_structs(text)
    names = []
    for m in re.finditer(r'\bint\s+(vkx_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S):
        params = [p.strip() for p in m.group(2).split(',') if p.strip()]
        if any('stride' in p.split()[-1] or 'pitch' in p.split()[-1] or set(re.findall(r'\w+', p)) & structs for p in params):
            names.append(m.group(1))
    return names


def _header_text(path=HEADER):
    with open(path) as f:
        return re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)


def struct_stride_fields(path=HEADER):
    """{struct type of vkx.h: the names of its fields that contain `stride`}"""
    out = {}
    for m in re.finditer(r'typedef\s+struct\s+\w+\s*\{([^}]*)\}\s*(\w+)\s*;', _header_text(path), flags=re.S):
        fields = [f for f in re.findall(r'\b(\w+)\s*(?:\[[^\]]*\])?\s*[,;]', m.group(1)) if 'stride' in f]
        if fields:
            out[m.group(2)] = fields
    return out


def struct_params(path=HEADER):
    """{export: the strided struct types among its parameters}"""
    structs = set(struct_stride_fields(path))
    out = {}
    for m in re.finditer(r'\bint\s+(vkx_\w+)\s*\(([^;]*?)\)\s*;', _header_text(path), flags=re.S):
        used = set(re.findall(r'\w+', m.group(2))) & structs
        if used:
            out[m.group(1)] = used
    return out


def descriptor_gaps(cases, path=HEADER):
    """The covered entry points with a strided struct parameter that no descriptor case of test_gpu_strides.py covers in full: a
    case counts only if its `descriptors` name, over the records of the struct, every strided field of it (but UNLAID_FIELDS),
    each on a plane that takes the layouts (a member of one of the case's groups).  `cases`: objects with entry, dev_name, host,
    groups and, for descriptor cases, descriptors."""
    fields, params = struct_stride_fields(path), struct_params(path)
    gaps = []
    for name in sorted(COVERED):
        for struct in sorted(params.get(name, ())):
            need = {f for f in fields[struct] if (name, struct, f) not in UNLAID_FIELDS}
            best = None
            for c in cases:
                if name != (c.dev_name if name.endswith('_dev') or name == c.dev_name else (c.entry if c.host else None)):
                    continue
                laid = {n for g in c.groups for n in g}
                have = {f for rec in getattr(c, 'descriptors', {}).get(struct, ()) for f, plane in rec.items() if plane in laid}
                if best is None or len(need - have) < len(best):
                    best = need - have
            if best is None or best:
                gaps.append(f'{name}: {struct} fields {sorted(best) if best is not None else sorted(need)} are laid out by no descriptor case')
    return gaps
