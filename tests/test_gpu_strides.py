"""The pitch contract of include/vkx.h for every strided entry point (tests/stride_table.py lists them).

Each case runs one entry point on planes laid out as
  dense      rows back to back, 256-byte aligned base
  off1..3    rows back to back, the base 1, 2 or 3 ELEMENTS past an aligned address
  pad        a pitch longer than the row (odd for uint8)
  roi        a window of a larger plane, starting at row 3, column 3
applied to each plane on its own (the others dense) and to all planes at once, and compares the result bit for bit with
the oracle (oracle/, tests/jpeg_restate.py, or numpy statements of the formulas vkx.h gives) on the dense input.  The one
exception is zoom_in_blur, whose oracle takes the operator's ratio / step and not the explicit sizes of the entry point:
its cases compare every layout with the dense host call, a differential check (test_gpu_pointwise::test_zoom_in_blur pins
the dense path to the oracle).  Every plane sits between guards of more than a row plus 4 KB: bytes of a
source outside its window are random, so a kernel that reads outside gives other values; bytes of a destination outside
its window are 0xA5 and must stay so.  Source planes must come back unchanged.

Entry points whose strides travel in descriptor structs (chain items, remap elements, layers, paint sets, noise planes) are
DescCase cases: the same layouts and schedules, one group per plane a descriptor names, and every run checks that the
descriptors it passed carried the strides of those layouts.  The chain cases run the fused kernel (whole 4-pixel groups,
ragged tails of 1, 2 and 3 columns, streak instance, remap alone, tiled noise drawn in the same call) and the staged kernels
(a 9-tap blur, which the fused plan declines) on laid-out sources, destinations and noise planes, two items per call.
"""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stride_table as T  # noqa: E402
import jpeg_restate as J  # noqa: E402

LAYOUTS = ('dense', 'off1', 'off2', 'off3', 'pad', 'roi')
PAGE = ('dense', 'off1', 'off3', 'pad', 'roi')        # page-scale planes: fewer runs
CANARY = 0xA5
VKX_ERR_INVALID = -1


class Buf:
    """One plane of `shape` / `dtype` placed in a guarded allocation by `layout` (device or host memory)."""

    def __init__(self, ctx, rng, data, shape, dtype, role, layout, host=False, guard_min=0):
        self.ctx, self.role, self.host = ctx, role, host
        dtype = np.dtype(dtype)
        self.shape, self.dtype = tuple(shape), dtype
        es = dtype.itemsize
        rows, w = self.shape[0], self.shape[1]
        cn = self.shape[2] if len(self.shape) == 3 else 1
        row_el = w * cn
        pitch_el, start_el = row_el, 0
        if layout.startswith('off'):
            start_el = int(layout[3:])
        elif layout == 'pad':
            pitch_el = row_el + (5 if es == 1 else 3)
        elif layout == 'roi':
            pitch_el = row_el + 7 * cn + (1 if es == 1 else 0)
            start_el = 3 * pitch_el + 3 * cn
        elif layout == 'short':
            pitch_el = row_el - 1
        elif layout == 'neg':
            pitch_el = -row_el
            start_el = (rows - 1) * row_el
        else:
            assert layout == 'dense', layout
        self.row_b, self.pitch_b = row_el * es, pitch_el * es
        guard = ((max(abs(self.pitch_b) + 4096, guard_min) + 255) // 256) * 256
        span = (start_el + max(rows - 1, 0) * max(pitch_el, 0) + row_el + (2 * pitch_el if layout == 'roi' else 0)) * es
        self.total = 2 * guard + max(span, (rows * row_el + start_el) * es)
        self.off = guard + start_el * es
        self.stride = pitch_el                # what the entry point takes: bytes for uint8, elements otherwise
        self.check_window = layout not in ('short', 'neg')
        if role == 'in':
            self.init = rng.integers(0, 256, self.total, dtype=np.uint8)
        else:
            self.init = np.full(self.total, CANARY, np.uint8)
        if data is not None and self.check_window:
            self.window(self.init)[...] = np.ascontiguousarray(data, dtype).reshape(rows, row_el).view(np.uint8)
        if host:
            self.mem = self.init.copy()
            self.p = self.mem.ctypes.data + self.off
        else:
            self.base = ctx.malloc(self.total)
            ctx.upload(self.base, self.init)
            self.p = self.base + self.off

    def window(self, buf):
        return as_strided(buf[self.off:], shape=(self.shape[0], self.row_b), strides=(self.pitch_b, 1), writeable=True)

    def finish(self):
        """(window content or None, list of problems); frees device memory"""
        if self.host:
            after = self.mem
        else:
            after = np.empty(self.total, np.uint8)
            self.ctx.download(self.base, after)
            self.ctx.free(self.base)
        problems, got = [], None
        self.untouched = bool((after == self.init).all())
        if self.check_window:
            got = self.window(after).copy().view(self.dtype).reshape(self.shape)
            if self.role == 'in':
                if not (after == self.init).all():
                    problems.append('source plane written')
            else:
                outside = after.copy()
                self.window(outside)[...] = self.window(self.init)
                bad = np.flatnonzero(outside != self.init)
                if bad.size:
                    problems.append(f'{bad.size} guard bytes overwritten (first at {int(bad[0]) - self.off} from the base)')
        elif not (after == self.init).all():
            problems.append('memory written by a refused call')
        return got, problems


class Case:
    """name, entry point (without _dev), planes {name: (data or None, shape, dtype, role)}, call(fn, P) -> rc or
    (rc, host outputs), want {plane or output name: array}."""

    def __init__(self, name, entry, planes, call, want, layouts=LAYOUTS, groups=None, refuse=None, host=False, extra=(),
                 dev_name=None):
        self.name, self.entry, self.planes, self.call, self.want = name, entry, planes, call, want
        self.layouts, self.host, self.refuse = layouts, host, refuse or {}
        self.groups = groups or [(n,) for n in planes if not planes[n][3].startswith('fixed')]
        self.extra = [dict(e) for e in extra]             # further schedules {group: layout}
        self.dev_name = dev_name or entry + '_dev'        # the device entry point (vkx_fill_u8_dev_host_layers has no host twin)

    def schedules(self):
        dense = {g: 'dense' for g in self.groups}
        yield dense
        for g in self.groups:
            for lay in self.layouts[1:]:
                yield {**dense, g: lay}
        if len(self.groups) > 1:
            for lay in self.layouts[1:]:
                yield {g: lay for g in self.groups}
            rot = self.layouts[1:]
            yield {g: rot[i % len(rot)] for i, g in enumerate(self.groups)}
            yield {g: (rot[(i + 2) % len(rot)] if i else 'dense') for i, g in enumerate(self.groups)}
        for e in self.extra:
            yield {**dense, **e}


class DescCase(Case):
    """A case of an entry point whose strides travel in descriptor structs (vkx_chain_item, vkx_elem, vkx_layer(_f32),
    vkx_paint_set, vkx_noise_plane).  `descriptors` {struct name of vkx.h: [{stride field: plane name} per record]} states which
    plane's layout each strided field of each record takes; the call hands the arrays it passes to note(), and run() checks
    that every stated field holds the stride of its plane's layout.  tests/stride_table.py descriptor_gaps() counts such a case
    as coverage of its entry point only if the stated fields are all the strided fields of the struct."""

    def __init__(self, *a, descriptors, **k):
        super().__init__(*a, **k)
        self.descriptors = descriptors

    def unlaid(self, notes, bufs):
        problems = []
        seen = dict(notes)
        for struct, records in self.descriptors.items():
            arr = seen.get(struct)
            if arr is None or len(arr) != len(records):
                problems.append(f'{struct}: the call noted {None if arr is None else len(arr)} records, the case states {len(records)}')
                continue
            for i, fields in enumerate(records):
                for f, plane in fields.items():
                    if int(getattr(arr[i], f)) != bufs[plane].stride:
                        problems.append(f'{struct}[{i}].{f} = {getattr(arr[i], f)} is not the stride of {plane} ({bufs[plane].stride})')
        return problems


_NOTES, _AFTER = [], []


def note(struct, array):
    """a call states the descriptor array it passes (DescCase)"""
    _NOTES.append((struct, array))


def after(fn):
    """a call leaves work for after the synchronisation: fn() -> list of problems (frees, flags and timings to read)"""
    _AFTER.append(fn)


def run(ctx, rng, case, sched, host=False, fn=None):
    lay = {}
    for g, lname in sched.items():
        for n in g:
            lay[n] = lname
    bufs = {}
    for n, (data, shape, dtype, role) in case.planes.items():
        data = data.value() if isinstance(data, _Later) else data
        shape = tuple(v.value() if isinstance(v, _Later) else v for v in shape)      # (a tile buffer's size comes from the library)
        # 'host_in': a plane the DEVICE entry point reads from host memory (the layers of vkx_fill_u8_dev_host_layers)
        bufs[n] = Buf(ctx, rng, data, shape, dtype, 'in' if role in ('fixed', 'host_in') else role, lay.get(n, 'dense'),
                      host=host or role == 'host_in')
    if fn is None:
        fn = getattr(__import__('vkit_amd._native', fromlist=['lib']).lib(), case.entry if host else case.dev_name)
    del _NOTES[:], _AFTER[:]
    res = case.call(fn, bufs)
    rc, outs = (res if isinstance(res, tuple) else (res, {}))
    ctx.sync()
    results, problems = dict(outs), []
    for hook in list(_AFTER):
        problems += hook() or []
    if isinstance(case, DescCase):
        problems += case.unlaid(_NOTES, bufs)
    del _NOTES[:], _AFTER[:]
    for n, b in bufs.items():
        got, pr = b.finish()
        problems += [f'{n}: {p}' for p in pr]
        if case.planes[n][3] in ('out', 'inout', 'fixed_out'):
            results[n] = got
    return rc, results, problems


def compare(case, results):
    bad = []
    for n, want in case.want.items():
        want = want.value() if isinstance(want, _Later) else want
        got = results.get(n)
        if got is None or got.shape != want.shape:
            bad.append(f'{n}: shape {None if got is None else got.shape} != {want.shape}')
            continue
        if want.dtype.kind == 'f':
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        else:
            same = got == want
        if not same.all():
            idx = np.argwhere(~same)
            bad.append(f'{n}: {idx.shape[0]} values differ, first at {tuple(idx[0])}: {got[tuple(idx[0])]} != {want[tuple(idx[0])]}')
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the table

def _img(rng, h, w, cn):
    return rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


def _cn(a):
    return a.shape[2] if a.ndim == 3 else 1


class _Later:
    """An expected value computed when a test first compares with it: building the table loads no library."""

    def __init__(self, fn, *args):
        self.fn, self.args, self.done = fn, args, None

    def value(self):
        if self.done is None:
            self.done = self.fn(*self.args)
        return self.done


later = _Later


class _Handle:
    """The default context's handle, looked up when an entry point is called (ctypes reads `_as_parameter_`)."""

    @property
    def _as_parameter_(self):
        from vkit_amd import _native as N
        return N.default_ctx().handle


def _blend(a, b, w0, w1, channels):
    """vkx.h vkx_blend_u8: uint8(clip(w0 * a + w1 * b, 0, 255)) in float32 (products rounded separately, truncation) on
    `channels`, b elsewhere"""
    a3, b3 = a.reshape(a.shape[0], a.shape[1], -1), b.reshape(b.shape[0], b.shape[1], -1)
    t = np.float32(w0) * a3.astype(np.float32) + np.float32(w1) * b3.astype(np.float32)
    out = b3.copy()
    for c in channels:
        out[:, :, c] = np.clip(t[:, :, c], 0, 255).astype(np.uint8)
    return out.reshape(b.shape)


def _fog(img, m, fog):
    """vkx.h vkx_fog_f32_u8: uint8(clip((1 - m) * px + m * fog[c], 0, 255)) in float32"""
    px = img.reshape(img.shape[0], img.shape[1], -1).astype(np.float32)
    t = (np.float32(1) - m)[:, :, None] * px + m[:, :, None] * fog[None, None, :]
    return np.clip(t, 0, 255).astype(np.uint8).reshape(img.shape)


def _sums(img, sel, sequential):
    """vkx.h vkx_sum_f32_u8: np.mean's float32 sums -- sequential over the pixels, or per channel pieces of 8 192 elements
    summed exactly and accumulated in float32"""
    flat = img.reshape(-1, img.shape[2] if img.ndim == 3 else 1)
    out = np.zeros(len(sel), np.float32)
    for k, c in enumerate(sel):
        v = flat[:, c]
        if sequential:
            out[k] = np.add.accumulate(v.astype(np.float32), dtype=np.float32)[-1]
        else:
            acc = np.float32(0)
            for i in range(0, v.size, 8192):
                acc = np.float32(acc + np.float32(int(v[i:i + 8192].sum(dtype=np.int64))))
            out[k] = acc
    return out


def _ellipse_streak(O, img, center, axes, thickness, color, alpha):
    """vkx.h vkx_ellipse_streak_u8: the ellipse outlines on a cleared mask, then Mask.fill_image(image, color, alpha)"""
    mask = np.zeros(img.shape[:2], np.uint8)
    for ax in axes:
        O.ellipse_outline(mask, center, tuple(int(v) for v in ax), thickness)
    out = img.copy()
    O.fill(out, (0, 0) + img.shape[:2], color if img.ndim == 3 else color[0], mask=mask, alpha=alpha)
    return out


def _filled(O, base, fills):
    out = base.copy()
    for box, value, kw in fills:
        O.fill(out, box, value, **kw)
    return out


def _outlined(O, mask, center, axes, thickness):
    out = mask.copy()
    for ax in axes:
        O.ellipse_outline(out, center, tuple(int(v) for v in ax), thickness)
    return out


def build_cases():
    """The table.  Building it loads no library: expected values are computed by the tests (_Later) and the context
    handle is looked up per call."""
    from vkit_amd import _native as N
    import oracle as O
    H = _Handle()
    rng = np.random.default_rng(20261015)
    cases = []
    u8, f32, i16, i32 = np.uint8, np.float32, np.int16, np.int32

    def add(*a, **k):
        cases.append(DescCase(*a, **k) if 'descriptors' in k else Case(*a, **k))

    # ---- resize: every interpolation code, uint8 1 / 3 / 4 channels and float32, both ways, the exact half, integer area
    small = [((37, 53), (29, 41)), ((37, 53), (61, 83)), ((38, 54), (19, 27)), ((36, 54), (12, 18)), ((5, 70), (3, 9))]
    for interp in range(7):
        for (sh, sw), (dh, dw) in small:
            if interp == 3 and (dh > sh or dw > sw):
                continue
            for cn in (1, 3, 4):
                src = _img(rng, sh, sw, cn)
                dshape = (dh, dw) + src.shape[2:]
                add(f'resize_u8 i{interp} cn{cn} {sh}x{sw}->{dh}x{dw}', 'vkx_resize_u8',
                    {'src': (src, src.shape, u8, 'in'), 'dst': (None, dshape, u8, 'out')},
                    lambda fn, P, sh=sh, sw=sw, cn=cn, dh=dh, dw=dw, i=interp: fn(
                        H, P['src'].p, sh, sw, cn, P['src'].stride, P['dst'].p, dh, dw, P['dst'].stride, i),
                    {'dst': later(O.resize, src, (dh, dw), interp)}, host=(interp == 2 and cn == 3 and sh == 37 and dh == 29))
            srcf = rng.random((sh, sw), dtype=np.float32) * 4 - 1
            add(f'resize_f32 i{interp} {sh}x{sw}->{dh}x{dw}', 'vkx_resize_f32',
                {'src': (srcf, srcf.shape, f32, 'in'), 'dst': (None, (dh, dw), f32, 'out')},
                lambda fn, P, sh=sh, sw=sw, dh=dh, dw=dw, i=interp: fn(
                    H, P['src'].p, sh, sw, P['src'].stride, P['dst'].p, dh, dw, P['dst'].stride, i),
                {'dst': later(O.resize, srcf, (dh, dw), interp)}, host=(interp == 4 and sh == 37 and dh == 61))
    # the cubic entry points themselves
    for cn in (1, 3):
        src = _img(rng, 45, 67, cn)
        dshape = (23, 33) + src.shape[2:]
        add(f'resize_cubic_u8 cn{cn}', 'vkx_resize_cubic_u8', {'src': (src, src.shape, u8, 'in'), 'dst': (None, dshape, u8, 'out')},
            lambda fn, P, cn=cn: fn(H, P['src'].p, 45, 67, cn, P['src'].stride, P['dst'].p, 23, 33, P['dst'].stride),
            {'dst': later(O.resize_cubic, src, (23, 33))})
    srcf = rng.random((45, 67), dtype=np.float32)
    add('resize_cubic_f32', 'vkx_resize_cubic_f32', {'src': (srcf, srcf.shape, f32, 'in'), 'dst': (None, (70, 101), f32, 'out')},
        lambda fn, P: fn(H, P['src'].p, 45, 67, P['src'].stride, P['dst'].p, 70, 101, P['dst'].stride),
        {'dst': later(O.resize_cubic, srcf, (70, 101))})
    # the row switches of the two tap forms (tests/resize_routes.py CENTRES): at 40 destination rows an interior tile needs
    # exactly 24, 25 (the two uint8 instances of the separable kernel), 40 and 41 (the last separable shape, the first direct one)
    # source rows; a generator of their own, so that the rows below keep their data
    brng = np.random.default_rng(20261019)
    for interp, heights in ((2, (52, 54, 96, 98)), (4, (42, 44, 85, 86))):
        for sh in heights:
            src = _img(brng, sh, 70, 3)
            add(f'resize_u8 i{interp} cn3 {sh}x70->40x67 (row switch)', 'vkx_resize_u8',
                {'src': (src, src.shape, u8, 'in'), 'dst': (None, (40, 67, 3), u8, 'out')},
                lambda fn, P, sh=sh, i=interp: fn(H, P['src'].p, sh, 70, 3, P['src'].stride, P['dst'].p, 40, 67, P['dst'].stride, i),
                {'dst': later(O.resize, src, (40, 67), interp)})
            srcf = brng.random((sh, 70), dtype=np.float32) * 4 - 1
            add(f'resize_f32 i{interp} {sh}x70->40x67 (row switch)', 'vkx_resize_f32',
                {'src': (srcf, srcf.shape, f32, 'in'), 'dst': (None, (40, 67), f32, 'out')},
                lambda fn, P, sh=sh, i=interp: fn(H, P['src'].p, sh, 70, P['src'].stride, P['dst'].p, 40, 67, P['dst'].stride, i),
                {'dst': later(O.resize, srcf, (40, 67), interp)})
    # page scale: the 24-row and 40-row separable forms and the direct kernels (cubic, lanczos4), the exact half, the integer
    # area kernel and the general area tables, the linear-exact tables, nearest and nearest-exact; dw % 4 = 1, 2, 3
    page = _img(rng, 1024, 1024, 3)
    page1, page4 = page[:, :, 0].copy(), _img(rng, 1024, 1024, 4)
    pagef = rng.random((1024, 1024), dtype=np.float32)
    for src, interp, (dh, dw), what in (
            (page, 2, (1023, 1021), '24-row separable'), (page, 2, (600, 602), '40-row separable'), (page, 2, (300, 299), 'direct'),
            (page4, 4, (1000, 998), 'lanczos separable'), (page1, 4, (400, 401), 'lanczos direct'),
            (page, 1, (512, 512), 'exact half'), (page, 1, (700, 703), 'linear tables'),
            (page, 3, (256, 256), 'area integer factor'), (page1, 3, (700, 701), 'area tables'),
            (page, 5, (700, 703), 'linear exact tables'), (page, 0, (1100, 1101), 'nearest'), (page, 6, (777, 779), 'nearest exact')):
        cn = _cn(src)
        add(f'resize_u8 page i{interp} cn{cn} ->{dh}x{dw} ({what})', 'vkx_resize_u8',
            {'src': (src, src.shape, u8, 'in'), 'dst': (None, (dh, dw) + src.shape[2:], u8, 'out')},
            lambda fn, P, cn=cn, dh=dh, dw=dw, i=interp: fn(H, P['src'].p, 1024, 1024, cn, P['src'].stride, P['dst'].p, dh, dw,
                                                            P['dst'].stride, i),
            {'dst': later(O.resize, src, (dh, dw), interp)}, layouts=PAGE)
    for interp, (dh, dw) in ((2, (600, 602)), (2, (300, 299)), (4, (1023, 1021)), (3, (256, 256))):
        add(f'resize_f32 page i{interp} ->{dh}x{dw}', 'vkx_resize_f32',
            {'src': (pagef, pagef.shape, f32, 'in'), 'dst': (None, (dh, dw), f32, 'out')},
            lambda fn, P, dh=dh, dw=dw, i=interp: fn(H, P['src'].p, 1024, 1024, P['src'].stride, P['dst'].p, dh, dw, P['dst'].stride, i),
            {'dst': later(O.resize, pagef, (dh, dw), interp)}, layouts=PAGE)

    # ---- blur and filters
    for cn, (h, w), k, sigma in ((3, (41, 67), 5, 1.3), (1, (64, 64), 3, 0.8), (4, (33, 130), 7, 2.0), (3, (130, 257), 9, 2.5)):
        img = _img(rng, h, w, cn)
        add(f'gaussian_blur cn{cn} {h}x{w} k{k}', 'vkx_gaussian_blur_u8',
            {'src': (img, img.shape, u8, 'in'), 'dst': (None, img.shape, u8, 'out')},
            lambda fn, P, h=h, w=w, cn=cn, k=k, s=sigma: fn(H, P['src'].p, h, w, cn, P['src'].stride, k, s, P['dst'].p, P['dst'].stride),
            {'dst': later(O.gaussian_blur, img, k, sigma)}, host=(cn == 3 and k == 5))
    for cn, (h, w), kern, what in ((3, (47, 61), O.defocus_kernel(3), 'defocus'), (1, (64, 128), O.motion_kernel(5, 30.0), 'motion'),
                                   (4, (29, 35), O.defocus_kernel(6), 'defocus large'),
                                   (3, (40, 72), np.asarray(rng.random((3, 5)), np.float32), 'random 3x5')):
        img = _img(rng, h, w, cn)
        kern = np.ascontiguousarray(kern, np.float32)
        add(f'filter2d {what} cn{cn} {h}x{w}', 'vkx_filter2d_u8',
            {'src': (img, img.shape, u8, 'in'), 'dst': (None, img.shape, u8, 'out')},
            lambda fn, P, h=h, w=w, cn=cn, kern=kern: fn(H, P['src'].p, h, w, cn, P['src'].stride, kern.ctypes.data, kern.shape[0],
                                                         kern.shape[1], P['dst'].p, P['dst'].stride),
            {'dst': later(O.filter2d, img, kern)}, host=(what == 'defocus'))

    # ---- sampling: remap (image and mask forms, float32), affine and perspective warps
    for cn, (sh, sw), (dh, dw) in ((3, (50, 70), (45, 77)), (1, (64, 64), (64, 64)), (4, (31, 47), (40, 33))):
        img = _img(rng, sh, sw, cn)
        yy, xx = np.mgrid[0:dh, 0:dw].astype(np.float32)
        mx = (xx * (sw / dw) + rng.normal(0, 2, (dh, dw)) - 1).astype(np.float32)
        my = (yy * (sh / dh) + rng.normal(0, 2, (dh, dw)) - 1).astype(np.float32)
        dshape = (dh, dw) + img.shape[2:]
        planes = {'src': (img, img.shape, u8, 'in'), 'mx': (mx, mx.shape, f32, 'in'), 'my': (my, my.shape, f32, 'in'),
                  'dst': (None, dshape, u8, 'out')}
        add(f'remap_u8 cn{cn}', 'vkx_remap_u8', planes,
            lambda fn, P, sh=sh, sw=sw, cn=cn, dh=dh, dw=dw: fn(H, P['src'].p, sh, sw, cn, P['src'].stride, P['mx'].p, P['my'].p,
                                                                P['mx'].stride, P['dst'].p, dh, dw, P['dst'].stride),
            {'dst': later(O.remap, img, mx, my)}, groups=[('src',), ('mx', 'my'), ('dst',)], host=(cn == 3))
        if cn == 1:
            mask = (img > 127).astype(np.uint8)
            add('remap_u8 mask', 'vkx_remap_u8', {**planes, 'src': (mask, mask.shape, u8, 'in')},
                lambda fn, P, sh=sh, sw=sw, dh=dh, dw=dw: fn(H, P['src'].p, sh, sw, 1, P['src'].stride, P['mx'].p, P['my'].p,
                                                             P['mx'].stride, P['dst'].p, dh, dw, P['dst'].stride),
                {'dst': later(O.remap, mask, mx, my)}, groups=[('src',), ('mx', 'my'), ('dst',)])
            plane = rng.random((sh, sw), dtype=np.float32)
            add('remap_f32', 'vkx_remap_f32', {**planes, 'src': (plane, plane.shape, f32, 'in'), 'dst': (None, (dh, dw), f32, 'out')},
                lambda fn, P, sh=sh, sw=sw, dh=dh, dw=dw: fn(H, P['src'].p, sh, sw, P['src'].stride, P['mx'].p, P['my'].p,
                                                             P['mx'].stride, P['dst'].p, dh, dw, P['dst'].stride),
                {'dst': later(O.remap, plane, mx, my)}, groups=[('src',), ('mx', 'my'), ('dst',)])
    A = np.array([[0.9, 0.21, -3.5], [-0.18, 1.07, 6.25]], np.float32).astype(np.float64)
    Pm = np.array([[1.02, 0.05, -2.0], [-0.03, 0.97, 3.0], [1e-4, -2e-4, 1.0]], np.float32).astype(np.float64)
    for kind, M in (('affine', A), ('perspective', Pm)):
        Mc = np.ascontiguousarray(M.reshape(-1))
        for cn in (1, 3, 4):
            img = _img(rng, 53, 71, cn)
            dw, dh = 66, 49
            add(f'warp_{kind}_u8 cn{cn}', f'vkx_warp_{kind}_u8',
                {'src': (img, img.shape, u8, 'in'), 'dst': (None, (dh, dw) + img.shape[2:], u8, 'out')},
                lambda fn, P, cn=cn, Mc=Mc: fn(H, P['src'].p, 53, 71, cn, P['src'].stride, Mc.ctypes.data, P['dst'].p, 49, 66,
                                               P['dst'].stride),
                {'dst': later(O.warp_affine if kind == 'affine' else O.warp_perspective, img, M, (dw, dh))},
                host=(kind == 'affine' and cn == 3))
        plane = rng.random((53, 71), dtype=np.float32)
        add(f'warp_{kind}_f32', f'vkx_warp_{kind}_f32', {'src': (plane, plane.shape, f32, 'in'), 'dst': (None, (49, 66), f32, 'out')},
            lambda fn, P, Mc=Mc: fn(H, P['src'].p, 53, 71, P['src'].stride, Mc.ctypes.data, P['dst'].p, 49, 66, P['dst'].stride),
            {'dst': later(O.warp_affine if kind == 'affine' else O.warp_perspective, plane, M, (66, 49))})

    # ---- pointwise family: the offset bases the dense-and-pitched test does not take
    h, w = 37, 53
    rgb = _img(rng, h, w, 3)
    simple = {'src': (rgb, rgb.shape, u8, 'in'), 'dst': (None, rgb.shape, u8, 'out')}
    add('color_shift', 'vkx_color_shift_rgb', simple,
        lambda fn, P, h=h, w=w: fn(H, P['src'].p, h, w, P['src'].stride, 37, P['dst'].p, P['dst'].stride),
        {'dst': later(O.color_shift_rgb, rgb, 37)}, host=True)
    add('rgb2hsv', 'vkx_cvt_rgb_hsv_u8', simple, lambda fn, P, h=h, w=w: fn(H, P['src'].p, h, w, P['src'].stride, 1, P['dst'].p, P['dst'].stride),
        {'dst': later(O.rgb2hsv_full, rgb)})
    add('brightness', 'vkx_brightness_shift_rgb', simple,
        lambda fn, P, h=h, w=w: fn(H, P['src'].p, h, w, P['src'].stride, 20, P['dst'].p, P['dst'].stride), {'dst': later(O.brightness_shift_rgb, rgb, 20)})
    add('color_balance', 'vkx_color_balance_rgb', simple,
        lambda fn, P, h=h, w=w: fn(H, P['src'].p, h, w, P['src'].stride, 0.4, P['dst'].p, P['dst'].stride), {'dst': later(O.color_balance_rgb, rgb, 0.4)})
    for cn in (1, 3, 4):
        img = _img(rng, h, w, cn)
        pl = {'src': (img, img.shape, u8, 'in'), 'dst': (None, img.shape, u8, 'out')}
        add(f'mean_shift cn{cn}', 'vkx_mean_shift_u8', pl,
            lambda fn, P, cn=cn, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, 40, 1, 128, 0, 0, P['dst'].p, P['dst'].stride),
            {'dst': later(O.mean_shift, img, 40, 128)})
        add(f'complement cn{cn}', 'vkx_pointwise_u8', pl,
            lambda fn, P, cn=cn, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, 0, -1, 0, 0, P['dst'].p, P['dst'].stride),
            {'dst': later(O.complement, img)})
        add(f'posterize cn{cn}', 'vkx_pointwise_u8', pl,
            lambda fn, P, cn=cn, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, 1, 5, 0, 0, P['dst'].p, P['dst'].stride),
            {'dst': later(O.posterization, img, 5)})
        if cn > 1:
            perm = [cn - 1 - c for c in range(cn)]
            code = sum(p << (2 * c) for c, p in enumerate(perm))
            add(f'permute cn{cn}', 'vkx_pointwise_u8', pl,
                lambda fn, P, cn=cn, code=code, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, 2, code, 0, 0, P['dst'].p, P['dst'].stride),
                {'dst': later(O.permute_channels, img, perm)})
        lut = rng.integers(0, 256, (cn, 256), dtype=np.uint8)
        want = img.copy().reshape(h, w, cn)
        for c in range(cn):
            want[:, :, c] = lut[c][want[:, :, c]]
        add(f'lut cn{cn}', 'vkx_apply_lut_u8', pl,
            lambda fn, P, cn=cn, lut=lut, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, lut.ctypes.data, 0, P['dst'].p, P['dst'].stride),
            {'dst': want.reshape(img.shape)})
        sel = rng.integers(0, 3, (h, w)).astype(np.uint8)
        add(f'impulse cn{cn}', 'vkx_impulse_noise_u8', {**pl, 'sel': (sel, sel.shape, u8, 'in')},
            lambda fn, P, cn=cn, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, P['sel'].p, P['sel'].stride, P['dst'].p, P['dst'].stride),
            {'dst': later(O.impulse_noise, img, sel)})
        hist = np.stack([np.bincount(img.reshape(h, w, cn)[:, :, c].ravel(), minlength=256) for c in range(cn)]).astype(np.int32)
        add(f'histogram cn{cn}', 'vkx_histogram_u8',
            {'src': (img, img.shape, u8, 'in'), 'hist': (np.zeros((cn, 256), np.int32), (cn, 256), i32, 'fixed_out')},
            lambda fn, P, cn=cn, h=h, w=w: fn(H, P['src'].p, h, w, cn, P['src'].stride, P['hist'].p), {'hist': hist})
    noise = rng.integers(-300, 300, (h, w, 3)).astype(np.int16)
    add('add_noise', 'vkx_add_noise_i16', {**simple, 'noise': (noise, noise.shape, i16, 'in')},
        lambda fn, P, h=h, w=w: fn(H, P['src'].p, h, w, 3, P['src'].stride, P['noise'].p, P['noise'].stride, P['dst'].p, P['dst'].stride),
        {'dst': later(O.add_noise_i16, rgb, noise)})

    # ---- composite and blend
    for cn in (1, 3, 4):
        a, b = _img(rng, 45, 83, cn), _img(rng, 45, 83, cn)
        add(f'blend cn{cn}', 'vkx_blend_u8', {'a': (a, a.shape, u8, 'in'), 'b': (b, b.shape, u8, 'in'), 'dst': (None, a.shape, u8, 'out')},
            lambda fn, P, cn=cn: fn(H, P['a'].p, P['a'].stride, P['b'].p, P['b'].stride, 45, 83, cn, 0.3, 0.7, 0b101, P['dst'].p,
                                    P['dst'].stride),
            {'dst': later(_blend, a, b, 0.3, 0.7, [c for c in (0, 2) if c < cn])}, host=(cn == 3))

    def u8_layers(P, cn, boxes):
        arr = (N.VkxLayer * 2)()
        (b0, b1) = boxes
        L = arr[0]
        L.up, L.left, L.height, L.width = b0
        L.mask, L.mask_stride = P['m0'].p, P['m0'].stride
        L.alpha, L.alpha_scalar = None, 1.0
        L.value, L.value_stride = P['v0'].p, P['v0'].stride
        L.mode = 0
        L = arr[1]
        L.up, L.left, L.height, L.width = b1
        L.mask = None
        L.alpha, L.alpha_stride_el = P['a1'].p, P['a1'].stride
        L.alpha_scalar = 1.0
        L.value = None
        for c in range(4):
            L.value_const[c] = 17 * (c + 3)
        L.mode = 0
        note('vkx_layer', arr)
        return arr
    two_layers = [{'mask_stride': 'm0', 'value_stride': 'v0'}, {'alpha_stride_el': 'a1'}]

    for cn in (1, 3, 4):
        h, w = 61, 97
        base = _img(rng, h, w, cn)
        b0, b1 = (5, 7, 33, 51), (20, 40, 40, 57)
        m0 = rng.integers(0, 2, b0[2:], dtype=np.uint8)
        v0 = _img(rng, b0[2], b0[3], cn)
        a1 = rng.random(b1[2:], dtype=np.float32)
        a1[::3] = 0
        fills = [(b0, v0, {'mask': m0}), (b1, tuple(17 * (c + 3) for c in range(cn)) if cn > 1 else 51, {'alpha': a1})]
        want = later(_filled, O, base, fills)
        planes = {'dst': (base, base.shape, u8, 'inout'), 'm0': (m0, m0.shape, u8, 'in'), 'v0': (v0, v0.shape, u8, 'in'),
                  'a1': (a1, a1.shape, f32, 'in')}
        add(f'fill_u8 cn{cn}', 'vkx_fill_u8', planes,
            lambda fn, P, cn=cn, b0=b0, b1=b1, h=h, w=w: fn(H, P['dst'].p, h, w, cn, P['dst'].stride, u8_layers(P, cn, (b0, b1)), 2),
            {'dst': want}, host=(cn == 3), descriptors={'vkx_layer': two_layers})
        # the same composite with the layer planes in HOST memory, gathered by the entry point itself
        add(f'fill_u8 host layers cn{cn}', 'vkx_fill_u8_dev_host_layers',
            {**planes, **{n: planes[n][:3] + ('host_in',) for n in ('m0', 'v0', 'a1')}},
            lambda fn, P, cn=cn, b0=b0, b1=b1, h=h, w=w: fn(H, P['dst'].p, h, w, cn, P['dst'].stride, u8_layers(P, cn, (b0, b1)), 2),
            {'dst': want}, dev_name='vkx_fill_u8_dev_host_layers', descriptors={'vkx_layer': two_layers})
        if cn == 3:
            base2 = _img(rng, h, w, cn)
            want2 = later(_filled, O, base2, fills)

            def batch(fn, P, b0=b0, b1=b1, h=h, w=w):
                layers = (N.VkxLayer * 4)()
                two = u8_layers(P, 3, (b0, b1))
                layers[0], layers[1], layers[2], layers[3] = two[0], two[1], two[0], two[1]
                del _NOTES[:]
                note('vkx_layer', layers)
                dsts = (ctypes.c_void_p * 2)(P['dst'].p, P['dst2'].p)
                begin = np.array([0, 2, 4], np.int32)
                return fn(H, dsts, 2, h, w, 3, P['dst'].stride, layers, begin.ctypes.data)
            add('fill_u8_batch', 'vkx_fill_u8_batch', {**planes, 'dst2': (base2, base2.shape, u8, 'inout')}, batch,
                {'dst': want, 'dst2': want2}, groups=[('dst', 'dst2'), ('m0',), ('v0',), ('a1',)],
                descriptors={'vkx_layer': two_layers * 2})
    hf, wf = 50, 70
    basef = rng.random((hf, wf), dtype=np.float32)
    bf = (4, 9, 30, 41)
    mf = rng.integers(0, 2, bf[2:], dtype=np.uint8)
    af = rng.random(bf[2:], dtype=np.float32)
    vf = rng.random(bf[2:], dtype=np.float32) * 10
    wantf = later(_filled, O, basef, [(bf, vf, {'mask': mf, 'alpha': af})])

    def fill_f32(fn, P):
        L = (N.VkxLayerF32 * 1)()
        L[0].up, L[0].left, L[0].height, L[0].width = bf
        L[0].mask, L[0].mask_stride = P['m'].p, P['m'].stride
        L[0].alpha, L[0].alpha_stride_el, L[0].alpha_scalar = P['a'].p, P['a'].stride, 1.0
        L[0].value, L[0].value_stride_el = P['v'].p, P['v'].stride
        L[0].mode = 0
        note('vkx_layer_f32', L)
        return fn(H, P['dst'].p, hf, wf, P['dst'].stride, L, 1)
    add('fill_f32', 'vkx_fill_f32', {'dst': (basef, basef.shape, f32, 'inout'), 'm': (mf, mf.shape, u8, 'in'),
                                     'a': (af, af.shape, f32, 'in'), 'v': (vf, vf.shape, f32, 'in')}, fill_f32, {'dst': wantf},
        descriptors={'vkx_layer_f32': [{'mask_stride': 'm', 'alpha_stride_el': 'a', 'value_stride_el': 'v'}]})

    # ---- streaks (in place)
    for cn in (1, 3, 4):
        img = _img(rng, 70, 90, cn)
        col = np.array([10, 200, 30, 40], np.uint8)
        add(f'line_streak cn{cn}', 'vkx_line_streak_u8', {'img': (img, img.shape, u8, 'inout')},
            lambda fn, P, cn=cn, col=col: fn(H, P['img'].p, 70, 90, cn, P['img'].stride, 2, 7, 3, 2, col.ctypes.data, 0.6, 1, 1),
            {'img': later(O.line_streak, img, 2, 7, 3, 2, tuple(int(c) for c in col[:cn]), 0.6, True, True)}, host=(cn == 3))
        axes = np.array([[20, 12], [35, 28]], np.int32)
        add(f'ellipse_streak cn{cn}', 'vkx_ellipse_streak_u8', {'img': (img, img.shape, u8, 'inout')},
            lambda fn, P, cn=cn, col=col, axes=axes: fn(H, P['img'].p, 70, 90, cn, P['img'].stride, 44, 33, axes.ctypes.data, 2, 2,
                                                        col.ctypes.data, 0.7),
            {'img': later(_ellipse_streak, O, img, (44, 33), axes, 2, tuple(int(c) for c in col[:cn]), 0.7)}, host=True)
    mask0 = (rng.random((70, 90)) < 0.02).astype(np.uint8) * 7
    axes = np.array([[20, 12], [35, 28], [3, 50]], np.int32)
    wantm = later(_outlined, O, mask0, (44, 33), axes, 3)
    add('ellipse_mask', 'vkx_ellipse_mask_u8', {'mask': (mask0, mask0.shape, u8, 'inout')},
        lambda fn, P: fn(H, P['mask'].p, P['mask'].stride, 70, 90, 44, 33, axes.ctypes.data, 3, 3), {'mask': wantm}, host=True)

    # ---- noise and effects
    for cn in (1, 3):
        img = _img(rng, 41, 59, cn)
        nz = rng.normal(0, 0.4, img.shape)
        add(f'speckle cn{cn}', 'vkx_speckle_noise_u8',
            {'src': (img, img.shape, u8, 'in'), 'noise': (nz, nz.shape, np.float64, 'in'), 'dst': (None, img.shape, u8, 'out')},
            lambda fn, P, cn=cn: fn(H, P['src'].p, 41, 59, cn, P['src'].stride, P['noise'].p, P['noise'].stride, P['dst'].p,
                                    P['dst'].stride),
            {'dst': later(O.speckle_noise, img, nz)}, host=(cn == 3))
        wt = rng.random((41, 59), dtype=np.float32)
        fog = np.array([200.0, 180.5, 90.25][:cn], np.float32)
        add(f'fog cn{cn}', 'vkx_fog_f32_u8',
            {'src': (img, img.shape, u8, 'in'), 'wt': (wt, wt.shape, f32, 'in'), 'dst': (None, img.shape, u8, 'out')},
            lambda fn, P, cn=cn, fog=fog: fn(H, P['src'].p, 41, 59, cn, P['src'].stride, P['wt'].p, P['wt'].stride, fog.ctypes.data,
                                             P['dst'].p, P['dst'].stride),
            {'dst': later(_fog, img, wt, fog)}, host=(cn == 3))
    for cn in (1, 3, 4):
        img = _img(rng, 40, 50, cn)
        py = rng.integers(0, 40, (33, 61)).astype(np.int32)
        px = rng.integers(0, 50, (33, 61)).astype(np.int32)
        add(f'gather cn{cn}', 'vkx_gather_u8',
            {'src': (img, img.shape, u8, 'in'), 'py': (py, py.shape, i32, 'in'), 'px': (px, px.shape, i32, 'in'),
             'dst': (None, (33, 61) + img.shape[2:], u8, 'out')},
            lambda fn, P, cn=cn: fn(H, P['src'].p, 40, 50, cn, P['src'].stride, P['py'].p, P['px'].p, P['py'].stride, P['dst'].p, 33,
                                    61, P['dst'].stride),
            {'dst': img[py, px]}, groups=[('src',), ('py', 'px'), ('dst',)], host=(cn == 3))
    for shape, std, seed in (((37, 29, 3), 10.0, 5), ((20, 33, 1), 3.0, 2 ** 40 + 7)):
        add(f'noise_normal_i16 {shape}', 'vkx_noise_normal_i16', {'dst': (None, shape, i16, 'out')},
            lambda fn, P, shape=shape, std=std, seed=seed: fn(H, P['dst'].p, P['dst'].stride, shape[0], shape[1], shape[2], std, seed),
            {'dst': later(lambda shape=shape, std=std, seed=seed: O.noise_normal_i16(shape, std, seed).reshape(shape))},
            refuse={'dst': ('off1', 'off2', 'off3')}, host=(shape[2] == 3))   # a dense plane must be 8-byte aligned (vkx.h)

    # ---- the rest: JPEG round trip, zoom-in blur, float32 sums, colour conversions
    for cn, (h, w), q in ((3, (37, 45), 75), (1, (33, 70), 30), (3, (64, 64), 95)):
        img = _img(rng, h, w, cn)
        add(f'jpeg cn{cn} {h}x{w} q{q}', 'vkx_jpeg_roundtrip_u8', {'src': (img, img.shape, u8, 'in'), 'dst': (None, img.shape, u8, 'out')},
            lambda fn, P, h=h, w=w, cn=cn, q=q: fn(H, P['src'].p, h, w, cn, P['src'].stride, P['dst'].p, P['dst'].stride, q),
            {'dst': later(J.jpeg_roundtrip, img, q)}, host=(cn == 3 and q == 75))
    for cn in (1, 3):
        img = _img(rng, 50, 62, cn)
        sizes = np.array([[55, 68], [61, 75]], np.int32)
        add(f'zoom_in_blur cn{cn}', 'vkx_zoom_in_blur_u8', {'src': (img, img.shape, u8, 'in'), 'dst': (None, img.shape, u8, 'out')},
            lambda fn, P, cn=cn, sizes=sizes: fn(H, P['src'].p, 50, 62, cn, P['src'].stride, sizes.ctypes.data, 2, 0.6, P['dst'].p,
                                                 P['dst'].stride),
            {'dst': later(N.zoom_in_blur, img, sizes, 0.6)}, host=(cn == 3))
    for cn, sel, seq in ((1, [0], 0), (3, [0, 2], 0), (3, [0, 1, 2], 1), (4, [1, 2, 3, 0], 1)):
        img = _img(rng, 67, 129, cn)
        chans = np.array(sel, np.int32)
        want = later(_sums, img, sel, seq)

        def summ(fn, P, cn=cn, chans=chans, seq=seq):
            out = np.zeros(len(chans), np.float32)
            rc = fn(H, P['src'].p, 67, 129, cn, P['src'].stride, chans.ctypes.data, len(chans), seq, out.ctypes.data)
            return rc, {'sums': out}
        add(f'sum_f32 cn{cn} seq{seq}', 'vkx_sum_f32_u8', {'src': (img, img.shape, u8, 'in')}, summ, {'sums': want}, host=True)
    h, w = 39, 57
    rgb, gray, rgba = _img(rng, h, w, 3), _img(rng, h, w, 1), _img(rng, h, w, 4)
    a255 = np.full((h, w, 1), 255, np.uint8)
    for code, src, out_cn, want in ((0, rgb, 3, later(O.rgb2hsv_full, rgb)), (1, rgb, 3, later(O.hsv2rgb_full, rgb)),
                                    (2, rgb, 3, later(O.rgb2hls_full, rgb)), (3, rgb, 3, later(O.hls2rgb_full, rgb)),
                                    (4, rgb, 1, later(O.rgb2gray, rgb)), (5, gray, 3, np.repeat(gray[:, :, None], 3, 2)),
                                    (6, rgba, 3, rgba[:, :, :3].copy()), (7, rgb, 4, np.concatenate([rgb, a255], 2)),
                                    (8, gray, 4, np.concatenate([np.repeat(gray[:, :, None], 3, 2), a255], 2)),
                                    (9, rgba, 1, later(O.rgb2gray, rgba[:, :, :3].copy()))):
        out_shape = (h, w) if out_cn == 1 else (h, w, out_cn)
        add(f'cvt_color {code}', 'vkx_cvt_color_u8', {'src': (src, src.shape, u8, 'in'), 'dst': (None, out_shape, u8, 'out')},
            lambda fn, P, code=code, h=h, w=w: fn(H, P['src'].p, h, w, P['src'].stride, code, P['dst'].p, P['dst'].stride),
            {'dst': want}, host=(code in (4, 5)))
    _descriptor_cases(add, N, O, H)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# entry points whose planes travel in descriptors or that paint: the chain, the multi-element remaps, the grid map, the polygon
# raster and paint, the batched noise planes

CHAIN_ENTRIES = ('vkx_chain_rgb_batch_dev', 'vkx_chain_rgb_batch_np_dev')
CHAIN_GRIDS = ((150, 171, 40), (131, 158, 41), (121, 112, 42))      # synthetic_grid(h, w, 16, 5.0, seed); the third: a 1-column tail
CHAIN_PAIRS = ((0, 1), (2, 0))                                      # the two items of a call
NP_STD = 11.0
# name -> blur ksize, hue, noise ('plane' / 'tiles' / None), streak, runs in k_chain_fused, blur radius of the fused plan
CHAIN_VARIANTS = {
    'grouped': (5, True, 'plane', False, True, 2),          # phase E on packed 4-pixel groups
    'streak': (5, True, 'plane', True, True, 2),            # streak instance: per-pixel phase E
    'remap only': (0, False, None, False, True, 0),
    # vkx_gaussian_blur_u8_dev takes 9 taps (the 'gaussian_blur cn3 130x257 k9' case); the fused plan stops at 7 (RMAX, fused.hip)
    'blur9 staged': (9, True, 'plane', False, False, None),
    'np tiles': (5, True, 'tiles', False, True, 2),
}


def tile_census(dv, dshape, radius):
    """(interior, border) tiles of a result that hold lattice cells, as k_chain_setup bins them for a blur of `radius`
    (test_gpu_chain_noise_groups._tile_census with the tile side of the radius: the 64-pixel window minus the halo, in whole
    4-pixel groups), and the columns of the ragged tail of the last tile column."""
    side = (64 - 2 * radius) & ~3
    dh, dw = dshape
    tiles_y, tiles_x = -(-dh // side), -(-dw // side)
    reached = np.zeros((tiles_y, tiles_x), bool)
    quads = np.stack([dv[:-1, :-1], dv[:-1, 1:], dv[1:, 1:], dv[1:, :-1]], 2).reshape(-1, 4, 2)
    for q in quads:
        xmin, xmax, ymin, ymax = int(q[:, 0].min()), int(q[:, 0].max()), int(q[:, 1].min()), int(q[:, 1].max())
        tx0, ty0 = max(xmin - radius, 0) // side, max(ymin - radius, 0) // side
        tx1, ty1 = min((xmax + radius) // side, tiles_x - 1), min((ymax + radius) // side, tiles_y - 1)
        if tx0 <= tx1 and ty0 <= ty1:
            reached[ty0:ty1 + 1, tx0:tx1 + 1] = True
    interior = border = 0
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            wx0, wy0 = tx * side - radius, ty * side - radius
            inside = wx0 >= 0 and wy0 >= 0 and wx0 + 64 <= dw and wy0 + 64 <= dh
            interior += bool(reached[ty, tx] and inside)
            border += bool(reached[ty, tx] and not inside)
    return interior, border, (dw % side) & 3


_CHAIN = None


def chain_inputs():
    """per lattice of CHAIN_GRIDS: source image, vertices, result shape, the extreme-value noise plane, and the seed of its stream"""
    global _CHAIN
    if _CHAIN is None:
        from test_gpu_parity import synthetic_grid
        from test_gpu_chain_noise_groups import _extreme_plane
        rng = np.random.default_rng(20261018)
        _CHAIN = []
        for k, (h, w, seed) in enumerate(CHAIN_GRIDS):
            sv, dv, dshape = synthetic_grid(h, w, 16, 5.0, seed=seed)
            _CHAIN.append(dict(image=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), sv=sv, dv=dv, dshape=dshape,
                               plane=_extreme_plane(tuple(dshape) + (3,), k), seed=9100 + k))
    return _CHAIN


_CHAIN_WANT = {}


def chain_want(O, g, variant):
    """the oracle chain remap -> gaussian_blur -> color_shift_rgb -> add_noise_i16 -> line_streak of lattice g"""
    key = (g, variant)
    if key not in _CHAIN_WANT:
        c = chain_inputs()[g]
        ksize, hue, noise, streak, _fused, _r = CHAIN_VARIANTS[variant]
        if ('remap', g) not in _CHAIN_WANT:
            _CHAIN_WANT['remap', g] = O.remap(c['image'], *O.grid_to_map(c['sv'], c['dv'], c['dshape']))
        out = _CHAIN_WANT['remap', g]
        if ksize > 1:
            if ('hued', g, ksize) not in _CHAIN_WANT:
                _CHAIN_WANT['hued', g, ksize] = O.color_shift_rgb(O.gaussian_blur(out, ksize, 1.0), 37)
            out = _CHAIN_WANT['hued', g, ksize]
        if noise == 'plane':
            out = O.add_noise_i16(out, c['plane'])
        elif noise == 'tiles':
            shape = tuple(c['dshape']) + (3,)
            out = O.add_noise_i16(out, np.round(np.random.default_rng(c['seed']).normal(0, NP_STD, shape)).astype(np.int16))
        if streak:
            out = O.line_streak(out, 2, 9, 3, 5, (10, 200, 30), 0.6, True, True)
        _CHAIN_WANT[key] = out
    return _CHAIN_WANT[key]


def tiles_bytes(n):
    """bytes of the tile buffer of a VKX_NP_NORMAL_TILES job of n samples (vkx_np_tiles_layout: no device needed)"""
    from vkit_amd import _native as N
    return N.np_tiles_layout(n)[4]


def chain_planes(pair, variant, noise_kinds=None):
    """the planes of a chain call on the lattices `pair`: s / d / n (plane noise) / t (tile buffer, dense by definition) per item"""
    noise = CHAIN_VARIANTS[variant][2]
    planes = {}
    for i, g in enumerate(pair):
        c = chain_inputs()[g]
        dh, dw = c['dshape']
        kind = noise_kinds[i] if noise_kinds else noise
        planes[f's{i}'] = (c['image'], c['image'].shape, np.uint8, 'in')
        planes[f'd{i}'] = (None, (dh, dw, 3), np.uint8, 'out')
        if kind == 'plane':
            planes[f'n{i}'] = (c['plane'], (dh, dw, 3), np.int16, 'in')
        elif kind == 'tiles':
            planes[f't{i}'] = (None, (1, _Later(tiles_bytes, dh * dw * 3)), np.uint8, 'fixed_out')
        planes[f'sv{i}'] = (c['sv'], c['sv'].shape, np.int32, 'fixed')
        planes[f'dv{i}'] = (c['dv'], c['dv'].shape, np.int32, 'fixed')
    return planes


def chain_call(fn, P, pair, variant, with_jobs=False, check_kernel=True):
    """vkx_chain_rgb_batch_dev(items) or vkx_chain_rgb_batch_np_dev(items, jobs): one item per lattice of `pair`, its noise
    whatever planes P holds for it (n: a plane, t: a tile buffer with its job)"""
    from vkit_amd import _native as N
    ksize, hue, _noise, streak, fused, _r = CHAIN_VARIANTS[variant]
    arr = (N.VkxChainItem * len(pair))()
    jobs = []
    for i, g in enumerate(pair):
        c = chain_inputs()[g]
        it = arr[i]
        it.src, it.dst, it.src_stride, it.dst_stride = P[f's{i}'].p, P[f'd{i}'].p, P[f's{i}'].stride, P[f'd{i}'].stride
        it.sh, it.sw = c['image'].shape[:2]
        it.dh, it.dw = c['dshape']
        it.src_vertices, it.dst_vertices = P[f'sv{i}'].p, P[f'dv{i}'].p
        it.rows, it.cols = c['sv'].shape[:2]
        if f'n{i}' in P:
            it.noise, it.noise_stride_el = P[f'n{i}'].p, P[f'n{i}'].stride
        elif f't{i}' in P:
            it.noise, it.noise_tiled = P[f't{i}'].p, 1
            jobs.append(N.np_job(N.NP_NORMAL_TILES, N.np_stream(np.random.default_rng(c['seed'])), it.dh * it.dw * 3, NP_STD,
                                 dst=P[f't{i}'].p))
        it.blur_sigma, it.blur_ksize = 1.0, ksize
        it.hue_delta, it.hue_enabled = 37, int(hue)
        if streak:
            it.streak_enabled, it.streak_thickness, it.streak_gap, it.streak_dash_thickness, it.streak_dash_gap = 1, 2, 9, 3, 5
            it.streak_enable_vert = it.streak_enable_hori = 1
            it.streak_color[0], it.streak_color[1], it.streak_color[2] = 10, 200, 30
            it.streak_alpha = 0.6
    note('vkx_chain_item', arr)
    ctx = N.default_ctx()
    ctx.set_timing(1)
    ctx.reset_timings()
    if with_jobs:
        job_arr = (N.VkxNpJob * len(jobs))(*jobs)
        results = (N.VkxNpResult * len(jobs))()
        rc = fn(_Handle(), arr, len(pair), job_arr, len(jobs), results)
    else:
        rc = fn(_Handle(), arr, len(pair))

    def done():
        launches = {name: count for name, (_ms, count) in ctx.timings().items() if count}
        ctx.set_timing(0)
        problems = []
        if rc == 0 and check_kernel and ('k_chain_fused' in launches) != fused:
            problems.append(f'k_chain_fused {"did not run" if fused else "ran"}: {sorted(launches)}')
        if rc == 0 and with_jobs:
            problems += [f'stream {k} was flagged {results[k].flags}' for k in range(len(jobs)) if results[k].flags]
        return problems
    after(done)
    return rc


POLY_H, POLY_W = 24, 40
# two overlapping quads, a bow tie, one polygon leaving the plane on each side (vertices at negative coordinates and beyond
# w / h), one wholly outside, one empty
POLYGONS = {
    'quad a': [(3, 2), (20, 3), (18, 14), (4, 12)], 'quad b': [(10, 6), (30, 8), (28, 20), (12, 18)],
    'bow tie': [(22, 2), (36, 12), (36, 2), (22, 12)],
    'left': [(-6, 5), (5, 4), (6, 10), (-4, 12)], 'right': [(34, 14), (47, 13), (45, 20), (35, 19)],
    'top': [(14, -5), (20, -4), (21, 3), (13, 4)], 'bottom': [(5, 18), (12, 19), (11, 30), (4, 28)],
    'outside': [(50, 30), (60, 30), (60, 40), (50, 40)], 'empty': [],
}


def poly_tables(names):
    """(points int32 [n, 2], offsets int32 [len + 1], values float32 [len]) of the polygons `names`, in that order"""
    pts = np.array([p for n in names for p in POLYGONS[n]], np.int32).reshape(-1, 2)
    offs = np.cumsum([0] + [len(POLYGONS[n]) for n in names]).astype(np.int32)
    values = (np.arange(len(names), dtype=np.float32) * 1.75 + 2.5).astype(np.float32)
    return pts, offs, values


def paint_want(names, base_mask=None, base_score=None):
    """test_gpu_composite._paint_reference (the oracle's fill_poly over each polygon's own box, clipped, the last one wins)
    over the given planes, or over zeros (the fresh entry points)"""
    from test_gpu_composite import _paint_reference
    _pts, _offs, values = poly_tables(names)
    live = [(np.array(POLYGONS[n], np.int32), values[k]) for k, n in enumerate(names) if POLYGONS[n]]
    if live:
        mask, score = _paint_reference((POLY_H, POLY_W), [p for p, _v in live], [v for _p, v in live])
    else:
        mask, score = np.zeros((POLY_H, POLY_W), np.uint8), np.zeros((POLY_H, POLY_W), np.float32)
    painted = mask == 1
    if base_mask is not None:
        mask = np.where(painted, 1, base_mask).astype(np.uint8)
    if base_score is not None:
        score = np.where(painted, score, base_score).astype(np.float32)
    return mask, score


def _descriptor_cases(add, N, O, H):
    from test_gpu_parity import synthetic_grid
    rng = np.random.default_rng(20261019)
    u8, f32, i16, i32 = np.uint8, np.float32, np.int16, np.int32

    # ---- chain items: every variant on both pairs of lattices; the two items take different layouts in the mixed schedules
    for variant, (_ksize, _hue, noise, _streak, _fused, _radius) in CHAIN_VARIANTS.items():
        for pair in CHAIN_PAIRS:
            tiles = noise == 'tiles'
            records = [{'src_stride': f's{i}', 'dst_stride': f'd{i}', **({'noise_stride_el': f'n{i}'} if noise == 'plane' else {})}
                       for i in range(2)]
            add(f'chain {variant} {pair[0]}+{pair[1]}', 'vkx_chain_rgb_batch_np' if tiles else 'vkx_chain_rgb_batch',
                chain_planes(pair, variant),
                lambda fn, P, pair=pair, variant=variant, tiles=tiles: chain_call(fn, P, pair, variant, with_jobs=tiles),
                {f'd{i}': later(chain_want, O, g, variant) for i, g in enumerate(pair)}, layouts=PAGE,
                descriptors={'vkx_chain_item': records})

    # ---- lattice and map remaps of four elements: uint8 x1 / x3 / x4 and float32 through one lattice (result 109 x 142: 2 x 3 tiles of 64)
    sh, sw = 100, 130
    sv, dv, (dh, dw) = synthetic_grid(sh, sw, 16, 5.0, seed=43)
    assert dh > 64 and dw > 64
    mats = {'u1': _img(rng, sh, sw, 1), 'u3': _img(rng, sh, sw, 3), 'u4': _img(rng, sh, sw, 4),
            'f': rng.random((sh, sw), dtype=np.float32) * 4 - 1}
    maps = later(lambda: O.grid_to_map(sv, dv, (dh, dw), want_owner=True))
    mx, my, owner = (later(lambda k=k: maps.value()[k]) for k in range(3))
    planes = {}
    for n, m in mats.items():
        planes[f's_{n}'] = (m, m.shape, m.dtype, 'in')
        planes[f'd_{n}'] = (None, (dh, dw) + m.shape[2:], m.dtype, 'out')
    lattice = {'sv': (sv, sv.shape, i32, 'fixed'), 'dv': (dv, dv.shape, i32, 'fixed')}

    def elems(P):
        arr = (N.VkxElem * len(mats))()
        for e, (n, m) in zip(arr, mats.items()):
            e.src, e.dst, e.src_stride, e.dst_stride = P[f's_{n}'].p, P[f'd_{n}'].p, P[f's_{n}'].stride, P[f'd_{n}'].stride
            e.cn, e.is_f32 = _cn(m), int(m.dtype == np.float32)
        note('vkx_elem', arr)
        return arr
    records = [{'src_stride': f's_{n}', 'dst_stride': f'd_{n}'} for n in mats]
    want = {f'd_{n}': later(lambda m=m: O.remap(m, mx.value(), my.value())) for n, m in mats.items()}
    add('grid_remap four elements', 'vkx_grid_remap', {**planes, **lattice},
        lambda fn, P: fn(H, elems(P), len(mats), sh, sw, P['sv'].p, P['dv'].p, sv.shape[0], sv.shape[1], dh, dw),
        want, layouts=PAGE, host=True, descriptors={'vkx_elem': records})
    add('remap_multi four elements', 'vkx_remap_multi',
        {**planes, 'mx': (mx, (dh, dw), f32, 'in'), 'my': (my, (dh, dw), f32, 'in')},
        lambda fn, P: fn(H, elems(P), len(mats), sh, sw, P['mx'].p, P['my'].p, P['mx'].stride, dh, dw),
        want, layouts=PAGE, host=True, groups=[(n,) for n in planes] + [('mx', 'my')], descriptors={'vkx_elem': records})
    add('grid_to_map with owner', 'vkx_grid_to_map',
        {'mx': (None, (dh, dw), f32, 'out'), 'my': (None, (dh, dw), f32, 'out'), 'owner': (None, (dh, dw), i32, 'fixed_out'), **lattice},
        lambda fn, P: fn(H, P['sv'].p, P['dv'].p, sv.shape[0], sv.shape[1], dh, dw, P['mx'].p, P['my'].p, P['mx'].stride, P['owner'].p),
        {'mx': mx, 'my': my, 'owner': owner}, layouts=PAGE, host=True, groups=[('mx', 'my')])

    # ---- polygon paint and raster on a 24 x 40 plane
    h, w = POLY_H, POLY_W
    names = ['quad a', 'quad b', 'bow tie', 'left', 'empty', 'right', 'top', 'bottom', 'outside']
    pts, offs, values = poly_tables(names)
    base_mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
    base_score = rng.random((h, w), dtype=np.float32) * 9 - 3
    painted = later(paint_want, names, base_mask, base_score)
    fresh = later(paint_want, names)
    add('paint_polys', 'vkx_paint_polys', {'mask': (base_mask, (h, w), u8, 'inout'), 'score': (base_score, (h, w), f32, 'inout')},
        lambda fn, P: fn(H, pts.ctypes.data, offs.ctypes.data, len(names), values.ctypes.data, P['mask'].p, P['mask'].stride,
                         P['score'].p, P['score'].stride, h, w),
        {'mask': later(lambda: painted.value()[0]), 'score': later(lambda: painted.value()[1])}, layouts=PAGE, host=True)
    for what in ('mask', 'score', 'both'):
        planes = {n: (None, (h, w), t, 'out') for n, t in (('mask', u8), ('score', f32)) if what in (n, 'both')}

        def paint_fresh(fn, P):
            m, s = P.get('mask'), P.get('score')
            return fn(H, pts.ctypes.data, offs.ctypes.data, len(names), values.ctypes.data, m.p if m else None, m.stride if m else 0,
                      s.p if s else None, s.stride if s else 0, h, w)
        add(f'paint_polys_fresh {what}', 'vkx_paint_polys_fresh', planes, paint_fresh,
            {n: later(lambda k=k: fresh.value()[k]) for k, n in enumerate(('mask', 'score')) if n in planes}, layouts=PAGE)
    # three sets in the bands of one ownership raster: set 0 leaves its band at the bottom, set 1 (mask only) at the top, set 2
    # has no polygon; neither may show in its neighbour
    set_names = (['quad a', 'bottom', 'right', 'quad b'], ['top', 'bow tie', 'empty', 'left'], [])
    set_tables = [poly_tables(n) for n in set_names]
    set_planes = {'m0': (None, (h, w), u8, 'out'), 's0': (None, (h, w), f32, 'out'), 'm1': (None, (h, w), u8, 'out'),
                  'm2': (None, (h, w), u8, 'out'), 's2': (None, (h, w), f32, 'out')}

    def paint_sets(fn, P):
        arr = (N.VkxPaintSet * 3)()
        for k, (S, (p, o, v)) in enumerate(zip(arr, set_tables)):
            S.n_polys = len(set_names[k])
            if S.n_polys:
                S.pts_host, S.poly_offsets_host, S.values_host = p.ctypes.data, o.ctypes.data, v.ctypes.data
            S.mask, S.mask_stride = P[f'm{k}'].p, P[f'm{k}'].stride
            if f's{k}' in P:
                S.score, S.score_stride_el = P[f's{k}'].p, P[f's{k}'].stride
        note('vkx_paint_set', arr)
        return fn(H, arr, 3, h, w)
    set_want = [later(paint_want, n) for n in set_names]
    add('paint_poly_sets_fresh three sets', 'vkx_paint_poly_sets_fresh', set_planes, paint_sets,
        {n: later(lambda n=n: set_want[int(n[1])].value()[n[0] == 's']) for n in set_planes}, layouts=PAGE,
        descriptors={'vkx_paint_set': [{'mask_stride': 'm0', 'score_stride_el': 's0'}, {'mask_stride': 'm1'},
                                       {'mask_stride': 'm2', 'score_stride_el': 's2'}]})
    # the raster itself ORs into a 0 / 1 plane; vertices inside the mask (vkx.h): a polygon touching all four borders, a single
    # point in the last corner, a horizontal segment on the last row.  The last case starts from zeros: the host form overwrites.
    sparse = (rng.random((h, w)) < 0.1).astype(np.uint8)
    for what, poly, base, host in (('four borders', [(0, 5), (20, 0), (w - 1, 12), (15, h - 1)], sparse, False),
                                   ('corner point', [(w - 1, h - 1)], sparse, False),
                                   ('last row segment', [(5, h - 1), (30, h - 1)], sparse, False),
                                   ('four borders from zeros', [(0, 5), (20, 0), (w - 1, 12), (15, h - 1)], np.zeros((h, w), u8), True)):
        pp = np.array(poly, np.int32)
        add(f'fill_poly_mask {what}', 'vkx_fill_poly_mask_u8', {'mask': (base, (h, w), u8, 'inout')},
            lambda fn, P, pp=pp: fn(H, pp.ctypes.data, len(pp), P['mask'].p, h, w, P['mask'].stride),
            {'mask': later(lambda pp=pp, base=base: base | O.fill_poly((h, w), pp))}, layouts=PAGE, host=host)

    # ---- the planes of a noise batch: sample counts 3, 1, 2 and 0 mod 4, the first over three workgroups, the third a single
    # row; a dense plane must be 8-byte aligned (vkx.h), so the offset layouts are refusals
    shapes = ((61, 45, 3), (21, 33, 1), (1, 38, 3), (8, 11, 4))
    seeds = (5, 2 ** 40 + 7, 2 ** 63 + 11, 77)

    def noise_batch(fn, P):
        arr = (N.VkxNoisePlane * len(shapes))()
        for k, (pl, shape) in enumerate(zip(arr, shapes)):
            pl.dst, pl.stride_el, (pl.h, pl.w, pl.cn), pl.seed = P[f'p{k}'].p, P[f'p{k}'].stride, shape, seeds[k]
        note('vkx_noise_plane', arr)
        return fn(H, arr, len(shapes), 12.5)
    add('noise_normal_i16_batch four planes', 'vkx_noise_normal_i16_batch', {f'p{k}': (None, s, i16, 'out') for k, s in enumerate(shapes)},
        noise_batch, {f'p{k}': later(lambda s=s, seed=seed: O.noise_normal_i16(s, 12.5, seed).reshape(s))
                      for k, (s, seed) in enumerate(zip(shapes, seeds))},
        layouts=PAGE, refuse={f'p{k}': ('off1', 'off3') for k in range(len(shapes))},
        extra=[{('p0',): 'pad', ('p1',): 'roi', ('p2',): 'pad'}, {('p0',): 'roi', ('p2',): 'roi', ('p3',): 'pad'}],
        descriptors={'vkx_noise_plane': [{'stride_el': f'p{k}'} for k in range(len(shapes))]})


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in build_cases()}
    return _CASES


def _applies(test_name, case):
    """the cases each table-driven test runs: every case for the layouts, the marked ones on host memory, the small ones for
    the stride refusals, the small entry points that cannot run in place for the overlap refusal"""
    if test_name == 'test_host_entry_points_on_pitched_host_memory':
        return case.host
    if test_name == 'test_short_and_negative_strides_are_refused':
        return 'page' not in case.name and any(case.planes[g[0]][1][0] > 1 for g in case.groups)
    if test_name == 'test_overlapping_source_and_destination_are_refused':
        return ('page' not in case.name and _cannot_run_in_place(case) and 'src' in case.planes and 'dst' in case.planes
                and case.planes['src'][1][0] > 1)
    return True


def pytest_generate_tests(metafunc):
    if 'case_name' in metafunc.fixturenames:
        name = metafunc.function.__name__
        metafunc.parametrize('case_name', sorted(n for n, c in cases().items() if _applies(name, c)))


@pytest.mark.gpu
def test_table_matches_stride_table():
    """every device entry point tests/stride_table.py claims has a case, and every host entry point a host case"""
    entries = {c.dev_name for c in cases().values()}
    hosts = {c.entry for c in cases().values() if c.host}
    assert T.COVERED_DEV <= entries, sorted(T.COVERED_DEV - entries)
    assert T.COVERED_HOST <= hosts, sorted(T.COVERED_HOST - hosts)
    assert {'vkx_' + e for e in _BAD} | set(CHAIN_ENTRIES) == T.REFUSAL_TESTED
    assert not T.descriptor_gaps(cases().values())


@pytest.mark.gpu
def test_layouts(case_name):
    from vkit_amd import _native as N
    case = cases()[case_name]
    ctx = N.default_ctx()
    rng = np.random.default_rng(zlib.crc32(case_name.encode()))
    failures = []
    for sched in case.schedules():
        tag = ', '.join(f'{"+".join(g)}={lay}' for g, lay in sched.items() if lay != 'dense') or 'dense'
        refused = any(lay in case.refuse.get(g[0], ()) for g, lay in sched.items())
        rc, results, problems = run(ctx, rng, case, sched)
        if refused:
            if rc != VKX_ERR_INVALID:
                failures.append(f'[{tag}] rc {rc}, expected a refusal')
            failures += [f'[{tag}] {p}' for p in problems]
            continue
        if rc != 0:
            failures.append(f'[{tag}] rc {rc}: {N.last_error()}')
            continue
        failures += [f'[{tag}] {p}' for p in problems + compare(case, results)]
    assert not failures, f'{case_name}:\n' + '\n'.join(failures[:30])


@pytest.mark.gpu
def test_host_entry_points_on_pitched_host_memory(case_name):
    """the non-_dev form on host buffers whose pitch exceeds the row (the pitched gather and copy-out of HostStage,
    vkit_amd/csrc/vkx_host_stage.h, or the host form's own plane copies)"""
    from vkit_amd import _native as N
    case = cases()[case_name]
    ctx = N.default_ctx()
    rng = np.random.default_rng(7)
    failures = []
    fn = getattr(N.lib(), case.entry)
    groups = case.groups
    for sched in ({g: 'pad' for g in groups}, {g: 'roi' for g in groups}, {g: 'off3' for g in groups}):
        rc, results, problems = run(ctx, rng, case, sched, host=True, fn=fn)
        tag = next(iter(sched.values()))
        if any(tag in case.refuse.get(g[0], ()) for g in groups):
            continue
        if rc != 0:
            failures.append(f'[{tag}] rc {rc}: {N.last_error()}')
            continue
        failures += [f'[{tag}] {p}' for p in problems + compare(case, results)]
    assert not failures, f'{case_name} (host):\n' + '\n'.join(failures[:30])


# ---- argument checks: strides shorter than a row or negative, and overlapping planes where the kernel cannot run in place

NOT_IN_PLACE = {'vkx_resize_u8', 'vkx_resize_f32', 'vkx_resize_cubic_u8', 'vkx_resize_cubic_f32', 'vkx_remap_u8', 'vkx_remap_f32',
                'vkx_warp_affine_u8', 'vkx_warp_affine_f32', 'vkx_warp_perspective_u8', 'vkx_warp_perspective_f32',
                'vkx_gaussian_blur_u8', 'vkx_filter2d_u8', 'vkx_gather_u8', 'vkx_jpeg_roundtrip_u8', 'vkx_zoom_in_blur_u8'}


def _cannot_run_in_place(case):
    if case.entry in NOT_IN_PLACE:
        return True
    if case.entry == 'vkx_cvt_color_u8':
        return int(case.name.split()[-1]) >= 4             # the codes that change the channel count
    return case.name.startswith('permute')


@pytest.mark.gpu
def test_short_and_negative_strides_are_refused(case_name):
    """every plane of more than one row, one at a time, with a stride one element short of its row and with a negative
    stride: VKX_ERR_INVALID, and no byte of any plane written"""
    from vkit_amd import _native as N
    case = cases()[case_name]
    ctx = N.default_ctx()
    rng = np.random.default_rng(3)
    failures = []
    for g in case.groups:
        if case.planes[g[0]][1][0] <= 1:
            continue
        for lay in ('short', 'neg'):
            rc, _, problems = run(ctx, rng, case, {g: lay})
            if rc != VKX_ERR_INVALID:
                failures.append(f'[{"+".join(g)}={lay}] rc {rc}, expected VKX_ERR_INVALID')
            failures += [f'[{"+".join(g)}={lay}] {p}' for p in problems]
    assert not failures, f'{case_name}:\n' + '\n'.join(failures)


@pytest.mark.gpu
def test_overlapping_source_and_destination_are_refused(case_name):
    """an entry point that cannot run in place refuses a destination whose bytes overlap the source's, not only an equal
    pointer: here a dense destination that ends inside the source's first row (the source's guard in front of it is as
    long as the destination); the source allocation stays as it was"""
    from vkit_amd import _native as N
    case = cases()[case_name]
    dst_shape = case.planes['dst'][1]
    dst_bytes = int(np.prod(dst_shape)) * np.dtype(case.planes['dst'][2]).itemsize
    ctx = N.default_ctx()
    rng = np.random.default_rng(4)
    bufs = {n: Buf(ctx, rng, d, s, t, 'inout' if n == 'src' else ('in' if r == 'in' else 'out'), 'dense',
                   guard_min=dst_bytes if n == 'src' else 0)
            for n, (d, s, t, r) in case.planes.items()}

    class Alias:
        p = bufs['src'].p + bufs['src'].row_b - dst_bytes    # the destination's last bytes are the source's first row
        stride = int(np.prod(dst_shape[1:]))
    P = dict(bufs, dst=Alias)
    res = case.call(getattr(N.lib(), case.entry + '_dev'), P)
    rc = res[0] if isinstance(res, tuple) else res
    ctx.sync()
    problems = []
    for n, b in bufs.items():
        got, pr = b.finish()
        problems += pr
        if n == 'src' and got is not None and not (got == case.planes['src'][0]).all():
            problems.append('source window written')
    assert rc == VKX_ERR_INVALID and not problems, (case_name, rc, problems)


# ---- the refusals of the entry points outside the layout table (polygon raster and paint, grid maps, multi-element remaps)

def _raster_calls():
    """name -> call(fn_name, P) for the strided entry points outside the table, with the planes each takes: planes
    {name: (shape, dtype)}; each plane in turn gets a short or negative stride"""
    from vkit_amd import _native as N
    H = _Handle()
    h, w = 24, 40
    pts = np.array([[3, 2], [30, 5], [20, 20], [5, 15]], np.int32)
    offs = np.array([0, 4], np.int32)
    vals = np.array([2.5], np.float32)
    lattice = np.array([[[0, 0], [w - 1, 0]], [[0, h - 1], [w - 1, h - 1]]], np.int32)

    def elems(P, is_f32):
        arr = (N.VkxElem * 2)()
        for i in range(2):
            e = arr[i]
            e.src, e.dst = P[f's{i}'].p, P[f'd{i}'].p
            e.src_stride, e.dst_stride = P[f's{i}'].stride, P[f'd{i}'].stride
            e.cn, e.is_f32 = (1, 1) if is_f32 else (3, 0)
        return arr

    def sets(P):
        arr = (N.VkxPaintSet * 1)()
        S = arr[0]
        S.pts_host, S.poly_offsets_host, S.n_polys, S.values_host = pts.ctypes.data, offs.ctypes.data, 1, vals.ctypes.data
        S.mask, S.mask_stride, S.score, S.score_stride_el = P['mask'].p, P['mask'].stride, P['score'].p, P['score'].stride
        return arr
    mask_score = {'mask': ((h, w), np.uint8), 'score': ((h, w), np.float32)}
    two = {'s0': ((h, w, 3), np.uint8), 'd0': ((h, w, 3), np.uint8), 's1': ((h, w, 3), np.uint8), 'd1': ((h, w, 3), np.uint8),
           'mx': ((h, w), np.float32), 'my': ((h, w), np.float32), 'sv': ((2, 2, 2), np.int32), 'dv': ((2, 2, 2), np.int32)}
    return {
        'fill_poly_mask_u8_dev': ({'mask': ((h, w), np.uint8)},
                                  lambda fn, P: fn(H, pts.ctypes.data, 4, P['mask'].p, h, w, P['mask'].stride)),
        'paint_polys_dev': (mask_score, lambda fn, P: fn(H, pts.ctypes.data, offs.ctypes.data, 1, vals.ctypes.data, P['mask'].p,
                                                         P['mask'].stride, P['score'].p, P['score'].stride, h, w)),
        'paint_polys_fresh_dev': (mask_score, lambda fn, P: fn(H, pts.ctypes.data, offs.ctypes.data, 1, vals.ctypes.data,
                                                               P['mask'].p, P['mask'].stride, P['score'].p, P['score'].stride, h, w)),
        'paint_poly_sets_fresh_dev': (mask_score, lambda fn, P: fn(H, sets(P), 1, h, w)),
        'grid_to_map_dev': ({'mx': ((h, w), np.float32), 'my': ((h, w), np.float32), 'sv': ((2, 2, 2), np.int32),
                             'dv': ((2, 2, 2), np.int32)},
                            lambda fn, P: fn(H, P['sv'].p, P['dv'].p, 2, 2, h, w, P['mx'].p, P['my'].p, P['mx'].stride, None)),
        # the second element is the bad one: the first must not have been launched either
        'remap_multi_dev': (two, lambda fn, P: fn(H, elems(P, False), 2, h, w, P['mx'].p, P['my'].p, P['mx'].stride, h, w)),
        'grid_remap_dev': (two, lambda fn, P: fn(H, elems(P, False), 2, h, w, P['sv'].p, P['dv'].p, 2, 2, h, w)),
        # host forms that copy their planes themselves
        'paint_polys': (mask_score, lambda fn, P: fn(H, pts.ctypes.data, offs.ctypes.data, 1, vals.ctypes.data, P['mask'].p,
                                                     P['mask'].stride, P['score'].p, P['score'].stride, h, w)),
        'fill_poly_mask_u8': ({'mask': ((h, w), np.uint8)}, lambda fn, P: fn(H, pts.ctypes.data, 4, P['mask'].p, h, w,
                                                                              P['mask'].stride)),
    }, lattice


# the planes whose stride each of them takes (my shares mx's stride; the first element of a multi-element remap is good)
_BAD = {'fill_poly_mask_u8_dev': ('mask',), 'paint_polys_dev': ('mask', 'score'), 'paint_polys_fresh_dev': ('mask', 'score'),
        'paint_poly_sets_fresh_dev': ('mask', 'score'), 'grid_to_map_dev': ('mx',), 'remap_multi_dev': ('s1', 'd1', 'mx'),
        'grid_remap_dev': ('s1', 'd1'), 'paint_polys': ('mask', 'score'), 'fill_poly_mask_u8': ('mask',)}


@pytest.mark.gpu
@pytest.mark.parametrize('entry', sorted(_BAD))
def test_raster_and_multi_element_entry_points_refuse_bad_strides(entry):
    """each plane in turn with a stride one element short of its row, and negative: VKX_ERR_INVALID, and no byte of any
    plane written (for the multi-element remaps the bad plane belongs to the second element: the first is not run either)"""
    from vkit_amd import _native as N
    calls, lattice = _raster_calls()
    planes, call = calls[entry]
    host = not entry.endswith('_dev')
    fn = getattr(N.lib(), 'vkx_' + entry)
    ctx = N.default_ctx()
    rng = np.random.default_rng(5)
    failures = []
    for bad in _BAD[entry]:
        for lay in ('short', 'neg'):
            bufs = {n: Buf(ctx, rng, lattice if n in ('sv', 'dv') else None, shape, dt, 'in' if n in ('sv', 'dv') else 'out',
                           lay if n == bad else 'dense', host=host)
                    for n, (shape, dt) in planes.items()}
            rc = call(fn, bufs)
            if not host:
                ctx.sync()
            for b in bufs.values():
                b.finish()
            written = [n for n, b in bufs.items() if not b.untouched]
            if rc != VKX_ERR_INVALID:
                failures.append(f'[{bad}={lay}] rc {rc}, expected VKX_ERR_INVALID')
            if written:
                failures.append(f'[{bad}={lay}] planes written: {written}')
    assert not failures, f'{entry}:\n' + '\n'.join(failures)


# ---- the chain: what its lattices exercise, and the refusals of its items

def test_chain_lattices_hold_interior_and_border_tiles_and_every_tail():
    """the three lattices of the chain cases, for the 5-tap plan (tile side 60) and the plan without blur (64): interior and
    border tiles in each, and ragged tails of 1, 2 and 3 columns among them (3 * dw is 2, 1 and 3 mod 4)"""
    for radius in sorted({v[5] for v in CHAIN_VARIANTS.values() if v[4]}):
        tails = set()
        for c in chain_inputs():
            interior, border, tail = tile_census(c['dv'], c['dshape'], radius)
            assert interior >= 1 and border >= 1, (radius, c['dshape'], interior, border)
            tails.add(tail)
        assert tails == {1, 2, 3}, (radius, tails)
    assert [c['dshape'] for c in chain_inputs()[:2]] == [(161, 186), (141, 171)]
    assert {3 * c['dshape'][1] % 4 for c in chain_inputs()} == {1, 2, 3}


def _chain_refusal_bufs(ctx, rng, planes, layouts, guard_min=None):
    return {n: Buf(ctx, rng, d.value() if isinstance(d, _Later) else d, tuple(v.value() if isinstance(v, _Later) else v for v in shape),
                   t, 'in' if r == 'fixed' else ('inout' if n in (guard_min or {}) else r), layouts.get(n, 'dense'),
                   guard_min=(guard_min or {}).get(n, 0))
            for n, (d, shape, t, r) in planes.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('entry', CHAIN_ENTRIES)
def test_chain_items_refuse_bad_strides_and_overlap(entry):
    """src, dst and the plane noise of the SECOND item in turn with a stride one element short of the row, and negative, then a
    second item whose dense dst ends inside its src's first row: VKX_ERR_INVALID, and no byte of any plane written -- the
    first item has not run, and with vkx_chain_rgb_batch_np_dev (whose first item takes the tile buffer of a stream job)
    nothing was drawn either"""
    from vkit_amd import _native as N
    with_jobs = entry.endswith('_np_dev')
    pair, variant = CHAIN_PAIRS[0], 'grouped'
    planes = chain_planes(pair, variant, noise_kinds=('tiles' if with_jobs else 'plane', 'plane'))
    fn = getattr(N.lib(), entry)
    ctx = N.default_ctx()
    rng = np.random.default_rng(6)
    failures = []

    def attempt(tag, bufs, P):
        del _NOTES[:], _AFTER[:]
        rc = chain_call(fn, P, pair, variant, with_jobs=with_jobs, check_kernel=False)
        ctx.sync()
        for hook in list(_AFTER):
            hook()
        del _NOTES[:], _AFTER[:]
        for b in bufs.values():
            b.finish()
        written = [n for n, b in bufs.items() if not b.untouched]
        if rc != VKX_ERR_INVALID:
            failures.append(f'[{tag}] rc {rc}, expected VKX_ERR_INVALID')
        if written:
            failures.append(f'[{tag}] planes written: {written}')
    for bad in ('s1', 'd1', 'n1'):
        for lay in ('short', 'neg'):
            bufs = _chain_refusal_bufs(ctx, rng, planes, {bad: lay})
            attempt(f'{bad}={lay}', bufs, bufs)
    # the construction of test_overlapping_source_and_destination_are_refused on the second item
    dst_shape = planes['d1'][1]
    dst_bytes = int(np.prod(dst_shape))
    bufs = _chain_refusal_bufs(ctx, rng, planes, {}, guard_min={'s1': dst_bytes})

    class Alias:
        p = bufs['s1'].p + bufs['s1'].row_b - dst_bytes
        stride = int(np.prod(dst_shape[1:]))
    attempt('d1 ends in the first row of s1', bufs, dict(bufs, d1=Alias))
    assert not failures, f'{entry}:\n' + '\n'.join(failures)
