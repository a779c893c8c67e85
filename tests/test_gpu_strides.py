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

    def __init__(self, name, entry, planes, call, want, layouts=LAYOUTS, groups=None, refuse=None, host=False):
        self.name, self.entry, self.planes, self.call, self.want = name, entry, planes, call, want
        self.layouts, self.host, self.refuse = layouts, host, refuse or {}
        self.groups = groups or [(n,) for n in planes if not planes[n][3].startswith('fixed')]

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


def run(ctx, rng, case, sched, host=False, fn=None):
    lay = {}
    for g, lname in sched.items():
        for n in g:
            lay[n] = lname
    bufs = {}
    for n, (data, shape, dtype, role) in case.planes.items():
        bufs[n] = Buf(ctx, rng, data, shape, dtype, 'in' if role == 'fixed' else role, lay.get(n, 'dense'), host=host)
    if fn is None:
        fn = getattr(__import__('vkit_amd._native', fromlist=['lib']).lib(), case.entry + ('' if host else '_dev'))
    res = case.call(fn, bufs)
    rc, outs = (res if isinstance(res, tuple) else (res, {}))
    if not host:
        ctx.sync()
    results, problems = dict(outs), []
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
        cases.append(Case(*a, **k))

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
        return arr

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
            {'dst': want}, host=(cn == 3))
        if cn == 3:
            base2 = _img(rng, h, w, cn)
            want2 = later(_filled, O, base2, fills)

            def batch(fn, P, b0=b0, b1=b1, h=h, w=w):
                layers = (N.VkxLayer * 4)()
                two = u8_layers(P, 3, (b0, b1))
                layers[0], layers[1], layers[2], layers[3] = two[0], two[1], two[0], two[1]
                dsts = (ctypes.c_void_p * 2)(P['dst'].p, P['dst2'].p)
                begin = np.array([0, 2, 4], np.int32)
                return fn(H, dsts, 2, h, w, 3, P['dst'].stride, layers, begin.ctypes.data)
            add('fill_u8_batch', 'vkx_fill_u8_batch', {**planes, 'dst2': (base2, base2.shape, u8, 'inout')}, batch,
                {'dst': want, 'dst2': want2}, groups=[('dst', 'dst2'), ('m0',), ('v0',), ('a1',)])
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
        return fn(H, P['dst'].p, hf, wf, P['dst'].stride, L, 1)
    add('fill_f32', 'vkx_fill_f32', {'dst': (basef, basef.shape, f32, 'inout'), 'm': (mf, mf.shape, u8, 'in'),
                                     'a': (af, af.shape, f32, 'in'), 'v': (vf, vf.shape, f32, 'in')}, fill_f32, {'dst': wantf})

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
    return cases


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
    entries = {c.entry + '_dev' for c in cases().values()}
    hosts = {c.entry for c in cases().values() if c.host}
    assert T.COVERED_DEV <= entries, sorted(T.COVERED_DEV - entries)
    assert T.COVERED_HOST <= hosts, sorted(T.COVERED_HOST - hosts)
    assert {'vkx_' + e for e in _BAD} == T.REFUSAL_TESTED


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
