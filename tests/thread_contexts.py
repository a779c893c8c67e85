"""Families, seeds, the rotation and the child scenario of tests/test_gpu_thread_contexts.py -- a helper, not a test.

INTEGRATION.md gives callers one sentence about threads: a vkx_ctx is not thread safe, use one per thread.  The scenario here holds
the library to it: four threads, each with a context of its own for its whole life, enter the library together, and every result
is compared with a reference computed serially on the main thread before any thread started (oracle, numpy itself for the
streams and rng.poisson, the restatements under tests/).  Thread hazards do not depend on size, so the planes are PLANE = 70 x 67
(one tile edge in either direction, no multiple of 4 or 64: BAND_SW / BAND_DW of tests/resize_routes.py) and, for the chain,
LARGE = 96 x 128.  Every (thread, family, round) has its own seed, so no two threads expect the same bytes and a result that
lands in another thread's context is a mismatch, not a coincidence.

  phase A   a threading.Barrier(4) per family, then all four make their FIRST call of that family: the window the lazily built
            one-time state lives in (ONE_TIME_STATE).  Host arrays in, host arrays out.
  phase B   F families, F steps, thread t runs family (s + t) mod F at step s, inputs resident on the device where the wrapper
            takes them, one ctx.sync() a step before the comparison; the rotation runs twice (ROUNDS_B), so every family is once
            cold and once warm on every context.
  phase C   what is thread-local stays so: the refusal text of N.last_error(), N.resident(), N.default_ctx().

A family is make(seed) -> case (inputs and case['want'], a list), queue(N, ctx, case, dev) -> handle (everything queued, nothing
waited for beyond what the wrapper itself waits for) and collect(N, handle) -> list, compared item by item with case['want'].
planned() counts the comparisons of every phase without a GPU; tests/test_thread_contexts_plan.py checks the lists on the CPU.
"""
import os
import sys
import threading
import traceback

import numpy as np
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

THREADS = 4
PLANE = (70, 67)
LARGE = (96, 128)
BASE_SEED = 20261019
ROUNDS_B = 2
BARRIER_TIMEOUT = 120        # seconds: a thread that died before a barrier must not hang the others
CUBIC, AREA, LANCZOS4 = 2, 3, 4
REFUSAL = 'INTER_AREA'       # in the text of the refusal of phase C (resize.hip: an AREA resize that enlarges)


class Declined:
    """what collect() returns for a poisson image the device declined: the flags, and whether the generator was left alone"""

    def __init__(self, flags, untouched):
        self.flags, self.untouched = flags, untouched


def _host(x):
    return np.array(x.host()) if hasattr(x, 'host') else np.asarray(x)


def _put(ctx, a, dev):
    return ctx.to_device(a) if dev else a


def _image(rng, shape=PLANE, cn=3):
    return rng.integers(0, 256, tuple(shape) + ((cn,) if cn else ()), dtype=np.uint8)


def _polygon(rng, shape, n=5):
    """n vertices (x, y) around a random centre, inside the plane"""
    h, w = shape
    cy, cx = rng.integers(h // 3, 2 * h // 3), rng.integers(w // 3, 2 * w // 3)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(0.3, 1.0, n) * (min(h, w) // 3 - 1)
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], -1)
    return np.clip(np.rint(pts), 0, (w - 1, h - 1)).astype(np.int32)


def _state_dict(rng):
    return rng.bit_generator.state


# ---- the families ----------------------------------------------------------------------------------------------------------

class EllipseMask:
    name, count = 'ellipse_mask', 2            # thickness 1 and 3

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        h, w = PLANE
        center = (int(rng.integers(w // 3, 2 * w // 3)), int(rng.integers(h // 3, 2 * h // 3)))
        axes = [(int(a), int(b)) for a, b in rng.integers(1, 45, (4, 2))]        # every arc step: sizes below 3, 10, 15 and above
        start = (rng.random(PLANE) < 0.01).astype(np.uint8) * 5                  # drawn onto, as cv.ellipse does
        want = []
        for thickness in (1, 3):
            m = start.copy()
            for a in axes:
                O.ellipse_outline(m, center, a, thickness)
            want.append(m)
        return dict(center=center, axes=axes, start=start, want=want)

    @staticmethod
    def queue(N, ctx, case, dev):
        # the wrapper takes a host plane only
        return [N.ellipse_mask(case['start'].copy(), case['center'], case['axes'], t, ctx=ctx) for t in (1, 3)]

    @staticmethod
    def collect(N, handle):
        return handle


class NpNormal:
    name, count = 'np_normal_i16', 2           # the values, the generator afterwards

    @staticmethod
    def make(seed):
        std = float(default_rng([seed, 1]).uniform(4, 20))
        r = default_rng(seed)
        assert 'PCG64' in type(r.bit_generator).__name__
        plane = np.round(r.normal(0, std, PLANE + (3,))).astype(np.int16)
        return dict(seed=seed, std=std, want=[plane, _state_dict(r)])

    @staticmethod
    def queue(N, ctx, case, dev):
        r = default_rng(case['seed'])
        assert N.np_stream(r) is not None
        with N.resident(dev):
            got = N.np_normal_i16(PLANE + (3,), case['std'], r, ctx=ctx)
        return got, r

    @staticmethod
    def collect(N, handle):
        got, r = handle
        if got is None:
            return ['the device declined the stream', _state_dict(r)]
        return [_host(got), _state_dict(r)]


class NpPoisson:
    name, count = 'np_poisson_u8', 2           # the values, the generator afterwards (declined: counted, the generator untouched)

    @staticmethod
    def make(seed):
        rng = default_rng([seed, 2])
        img = _image(rng)
        img[:8] = rng.integers(0, 12, img[:8].shape)        # lam = 0 and the multiplication method below 10 beside PTRS
        r = default_rng(seed)
        want = np.clip(r.poisson(img.astype(np.float32)), 0, 255).astype(np.uint8)
        return dict(seed=seed, img=img, want=[want, _state_dict(r)])

    @staticmethod
    def queue(N, ctx, case, dev):
        r = default_rng(case['seed'])
        before = _state_dict(r)
        got = N.np_poisson_u8(_put(ctx, case['img'], dev), r, ctx=ctx)
        return got, r, N.np_poisson_last_flags(), before

    @staticmethod
    def collect(N, handle):
        got, r, flags, before = handle
        if got is None:
            d = Declined(flags, _state_dict(r) == before)
            return [d, d]
        return [_host(got), _state_dict(r)]


class ColorShift:
    name, count = 'color_shift_rgb', 1

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        img, delta = _image(rng), int(rng.integers(1, 255))
        return dict(img=img, delta=delta, want=[O.color_shift_rgb(img, delta)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.color_shift_rgb(_put(ctx, case['img'], dev), case['delta'], ctx=ctx)

    @staticmethod
    def collect(N, handle):
        return [_host(handle)]


class Resize:
    name, count = 'resize', 2                  # CUBIC and LANCZOS4 at one geometry: shrunk in y, enlarged in x
    DSIZE = (45, 83)

    @staticmethod
    def make(seed):
        import oracle as O
        img = _image(default_rng(seed))
        return dict(img=img, want=[O.resize(img, Resize.DSIZE, code) for code in (CUBIC, LANCZOS4)])

    @staticmethod
    def queue(N, ctx, case, dev):
        src = _put(ctx, case['img'], dev)
        return [N.resize(src, Resize.DSIZE, code, ctx=ctx) for code in (CUBIC, LANCZOS4)]

    @staticmethod
    def collect(N, handle):
        return [_host(x) for x in handle]


class GaussianBlur:
    name, count = 'gaussian_blur', 1

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        img, sigma = _image(rng), float(rng.uniform(0.7, 2.0))
        return dict(img=img, sigma=sigma, want=[O.gaussian_blur(img, 5, sigma)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.gaussian_blur(_put(ctx, case['img'], dev), 5, case['sigma'], ctx=ctx)

    @staticmethod
    def collect(N, handle):
        return [_host(handle)]


def lattice(rng, shape, step=15, jitter=4):
    """a regular lattice over `shape` and a jittered copy of it: (src vertices, dst vertices, destination shape)"""
    h, w = shape
    ys = list(range(0, h, step)) + ([h - 1] if (h - 1) % step else [])
    xs = list(range(0, w, step)) + ([w - 1] if (w - 1) % step else [])
    sv = np.array([[(x, y) for x in xs] for y in ys], np.int32)
    dv = (sv + rng.integers(-jitter, jitter + 1, sv.shape)).astype(np.int32)
    dv[..., 0] -= dv[..., 0].min()
    dv[..., 1] -= dv[..., 1].min()
    return sv, dv, (int(dv[..., 1].max()) + 1, int(dv[..., 0].max()) + 1)


class Remap:
    name, count = 'remap', 1                   # through a small lattice map

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        img = _image(rng)
        sv, dv, dshape = lattice(rng, PLANE)
        mx, my = O.grid_to_map(sv, dv, dshape)
        return dict(img=img, sv=sv, dv=dv, dshape=dshape, want=[O.remap(img, mx, my)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.grid_remap([_put(ctx, case['img'], dev)], case['sv'], case['dv'], case['dshape'], ctx=ctx)[0]

    @staticmethod
    def collect(N, handle):
        return [_host(handle)]


class WarpAffine:
    name, count = 'warp_affine', 1
    DSIZE_WH = (73, 61)

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        img = _image(rng)
        a, s = float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.8, 1.25))
        M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-6, 10)], [s * np.sin(a), s * np.cos(a), rng.uniform(-6, 10)]])
        return dict(img=img, M=M, want=[O.warp_affine(img, M, WarpAffine.DSIZE_WH)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.warp_affine(_put(ctx, case['img'], dev), case['M'], WarpAffine.DSIZE_WH, ctx=ctx)

    @staticmethod
    def collect(N, handle):
        return [_host(handle)]


class FillPolyMask:
    name, count = 'fill_poly_mask', 1

    @staticmethod
    def make(seed):
        import oracle as O
        pts = _polygon(default_rng(seed), PLANE, 7)
        return dict(pts=pts, want=[O.fill_poly(PLANE, pts)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.fill_poly_mask(PLANE, case['pts'], ctx=ctx)          # always a host array

    @staticmethod
    def collect(N, handle):
        return [np.array(handle)]


class PaintPolys:
    name, count = 'paint_polys', 2             # the mask and the score plane of two polygons, the later one wins

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        polygons = [_polygon(rng, PLANE, 5), _polygon(rng, PLANE, 6)]
        values = [float(v) for v in rng.uniform(0.5, 9.0, 2).astype(np.float32)]
        mask, score = np.zeros(PLANE, np.uint8), np.zeros(PLANE, np.float32)
        for polygon, value in zip(polygons, values):
            inside = O.fill_poly(PLANE, polygon).astype(bool)
            mask[inside] = 1
            score[inside] = value
        return dict(polygons=polygons, values=values, want=[mask, score])

    @staticmethod
    def queue(N, ctx, case, dev):
        if dev:
            mask, score = N.dev_zeros(PLANE, np.uint8, ctx), N.dev_zeros(PLANE, np.float32, ctx)
        else:
            mask, score = np.zeros(PLANE, np.uint8), np.zeros(PLANE, np.float32)
        N.paint_polys(case['polygons'], values=case['values'], mask=mask, score=score, ctx=ctx)
        return mask, score

    @staticmethod
    def collect(N, handle):
        return [_host(x) for x in handle]


class SetMask:
    name, count = 'set_mask', 1                # the element layer: Mask.from_polygons in DISTINCT mode

    @staticmethod
    def make(seed):
        import element_sets_restate as R
        rng = default_rng(seed)
        polygons = [_polygon(rng, PLANE, n) for n in (4, 5, 6)]
        return dict(polygons=polygons, want=[R.set_mask(R.POLYGONS, polygons, PLANE, 'distinct')])

    @staticmethod
    def queue(N, ctx, case, dev):
        # the element layer has no ctx argument: it runs on the calling thread's N.default_ctx(), one per thread like `ctx`
        import vkit_amd.element as E
        polygons = [E.Polygon.from_xy_pairs([(int(x), int(y)) for x, y in p]) for p in case['polygons']]
        with N.resident(dev):
            return E.Mask.from_polygons(PLANE, polygons, E.ElementSetOperationMode.DISTINCT)

    @staticmethod
    def collect(N, handle):
        return [np.array(handle.mat)]


class Fill:
    name, count = 'fill', 1                    # two layers: constant under a mask with a scalar alpha, then a plane under an alpha plane

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        dst = _image(rng)
        box1, box2 = (3, 5, 40, 50), (20, 11, 47, 53)
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        mask1 = (rng.random(box1[2:]) < 0.6).astype(np.uint8)
        alpha1 = float(rng.uniform(0.2, 0.9))
        value2 = _image(rng, box2[2:])
        alpha2 = rng.random(box2[2:], dtype=np.float32)
        want = dst.copy()
        O.fill(want, box1, color, mask=mask1, alpha=alpha1)
        O.fill(want, box2, value2, alpha=alpha2)
        return dict(dst=dst, layers=[(box1, color, mask1, alpha1), (box2, value2, None, alpha2)], want=[want])

    @staticmethod
    def queue(N, ctx, case, dev):
        dst = ctx.to_device(case['dst']) if dev else case['dst'].copy()
        layers = [N.make_layer(box, 3, value, mask=mask, alpha=alpha) for box, value, mask, alpha in case['layers']]
        return N.fill(dst, layers, ctx=ctx)

    @staticmethod
    def collect(N, handle):
        return [_host(handle)]


class MeanF32:
    name, count = 'mean_f32_u8', 1             # numpy's own np.mean of the float32 copy, per channel

    @staticmethod
    def make(seed):
        img = _image(default_rng(seed))
        return dict(img=img, want=[np.mean(img.astype(np.float32).reshape(-1, 3), axis=0)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.mean_f32_u8(_put(ctx, case['img'], dev), None, ctx=ctx)

    @staticmethod
    def collect(N, handle):
        return ['the device path was not taken' if handle is None else np.asarray(handle)]


class Jpeg:
    name, count = 'jpeg_roundtrip', 1          # quality 30

    @staticmethod
    def make(seed):
        import jpeg_restate as J
        img = _image(default_rng(seed))
        return dict(img=img, want=[J.jpeg_roundtrip(img, 30)])

    @staticmethod
    def queue(N, ctx, case, dev):
        return N.jpeg_roundtrip(_put(ctx, case['img'], dev), 30, ctx=ctx)

    @staticmethod
    def collect(N, handle):
        return [_host(handle)]


class Chain:
    name, count = 'chain_batch', 2             # two 96 x 128 images of one ChainBatch: remap, blur, hue, the numpy-stream noise
    STD = 9.0

    @staticmethod
    def make(seed):
        import oracle as O
        rng = default_rng(seed)
        images, grids, want = [], [], []
        for k in range(2):
            image = _image(rng, LARGE)
            sv, dv, dshape = lattice(rng, LARGE)
            mx, my = O.grid_to_map(sv, dv, dshape)
            base = O.color_shift_rgb(O.gaussian_blur(O.remap(image, mx, my), 5, 1.0), 37)
            plane = np.round(default_rng([seed, 7, k]).normal(0, Chain.STD, tuple(dshape) + (3,))).astype(np.int16)
            images.append(image)
            grids.append((sv, dv, dshape))
            want.append(O.add_noise_i16(base, plane))
        return dict(seed=seed, images=images, grids=grids, want=want)

    @staticmethod
    def queue(N, ctx, case, dev):
        from types import SimpleNamespace
        from vkit_amd.batch import ChainBatch
        batch = ChainBatch(ctx)
        for k, (image, (sv, dv, dshape)) in enumerate(zip(case['images'], case['grids'])):
            state = SimpleNamespace(result_shape=dshape, src_image_grid=SimpleNamespace(vertices=sv),
                                    dst_image_grid=SimpleNamespace(vertices=dv))
            batch.add(image, state, blur_sigma=1.0, hue_delta=37, noise_std=Chain.STD, noise_rng=default_rng([case['seed'], 7, k]))
        batch.run()
        return batch

    @staticmethod
    def collect(N, handle):
        try:
            return [np.array(handle.result(k)) for k in range(2)]
        finally:
            handle.close()


FAMILIES_A = (EllipseMask, NpNormal, NpPoisson, ColorShift, Resize)
FAMILIES_B = FAMILIES_A + (GaussianBlur, Remap, WarpAffine, FillPolyMask, PaintPolys, SetMask, Fill, MeanF32, Jpeg, Chain)
# the one-time state behind the first call of a phase A family
ONE_TIME_STATE = {'ellipse_mask': 'SinTable, process-wide (vkx_host_tables.h)',
                  'np_normal_i16': 'PCG64 jump tables, process-wide (vkx_host_tables.h); NpTabs per context',
                  'np_poisson_u8': "poisson.hip's tables, process-wide behind a std::once_flag",
                  'color_shift_rgb': 'HSV tables per context',
                  'resize': 'resize table cache per context'}


def rotation(step, thread, n_families=len(FAMILIES_B)):
    """the index of the family thread `thread` runs at step `step` of phase B"""
    return (step + thread) % n_families


def seed_of(thread, family, round_):
    """round 0: phase A; 1 .. ROUNDS_B: the rotations of phase B; ROUNDS_B + 1: phase C"""
    return [BASE_SEED, thread, [f.name for f in FAMILIES_B].index(family.name), round_]


# phase C: thread 0 names the refusal; threads 1 .. 3 a correct color_shift_rgb and no refusal in their text; threads 1 and 2 the
# kind of array inside / outside N.resident(True); every thread the same default context twice; the main thread: four distinct ones
PLAN_C = 1 + 2 * (THREADS - 1) + 2 + THREADS + 1


def planned():
    """{phase: comparisons}, counted from the lists alone"""
    return {'A': THREADS * sum(f.count for f in FAMILIES_A),
            'B': THREADS * ROUNDS_B * sum(f.count for f in FAMILIES_B),
            'C': PLAN_C}


def planned_interleaved():
    """the comparisons of the two-contexts-on-one-thread test: A alone, A then B, B then A, A alone again"""
    return (1 + 2 + 2 + 1) * sum(f.count for f in FAMILIES_B)


# ---- the comparison --------------------------------------------------------------------------------------------------------

def same(got, want):
    """None when equal (arrays: dtype, shape and every byte), else a short description"""
    if isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray):
            return f'{got!r} instead of an array'
        if got.dtype != want.dtype or got.shape != want.shape:
            return f'{got.dtype} {got.shape} != {want.dtype} {want.shape}'
        if got.tobytes() != want.tobytes():
            diff = np.argwhere(np.atleast_1d(got != want))
            first = tuple(int(v) for v in diff[0]) if len(diff) else ()
            return f'{len(diff)} values differ, first at {first}'
        return None
    return None if got == want else f'{str(got)[:200]} != {str(want)[:200]}'


class Tally:
    """what one thread (or the interleaved test) has compared: counts per phase, failures as strings"""

    def __init__(self, who):
        self.who, self.compared, self.declined, self.failures = who, {}, 0, []

    def fail(self, phase, what):
        self.failures.append(f'{self.who} phase {phase}: {what}')

    def check(self, phase, ok, what):
        self.compared[phase] = self.compared.get(phase, 0) + 1
        if not ok:
            self.fail(phase, what)

    def compare(self, phase, family, got, want, tag=''):
        if len(got) != len(want):
            self.fail(phase, f'{family.name} {tag}: {len(got)} results for {len(want)} references')
            return
        for i, (g, w) in enumerate(zip(got, want)):
            self.compared[phase] = self.compared.get(phase, 0) + 1
            if isinstance(g, Declined):
                self.declined += i == 0
                if not g.flags or not g.untouched:
                    self.fail(phase, f'{family.name} {tag}: declined with flags {g.flags}, generator untouched: {g.untouched}')
                continue
            diff = same(g, w)
            if diff:
                self.fail(phase, f'{family.name} {tag} result {i}: {diff}')

    def guarded(self, phase, what, fn):
        """fn() with any exception turned into a failure of this tally"""
        try:
            return fn()
        except Exception:
            self.fail(phase, f'{what}: ' + traceback.format_exc()[-1500:])
            return None


def run_family(N, ctx, family, case, dev, tally, phase, tag=''):
    def body():
        handle = family.queue(N, ctx, case, dev)
        ctx.sync()
        tally.compare(phase, family, family.collect(N, handle), case['want'], tag)
    tally.guarded(phase, f'{family.name} {tag}', body)


def expectations():
    """every case of phases A, B and C: {(thread, family name, round): case}, computed serially"""
    cases = {}
    for t in range(THREADS):
        for f in FAMILIES_A:
            cases[t, f.name, 0] = f.make(seed_of(t, f, 0))
        for r in range(1, ROUNDS_B + 1):
            for f in FAMILIES_B:
                cases[t, f.name, r] = f.make(seed_of(t, f, r))
        cases[t, ColorShift.name, ROUNDS_B + 1] = ColorShift.make(seed_of(t, ColorShift, ROUNDS_B + 1))
    return cases


# ---- the four threads --------------------------------------------------------------------------------------------------------

def _wait(barrier, tally, phase, what):
    try:
        barrier.wait(BARRIER_TIMEOUT)
    except threading.BrokenBarrierError:
        tally.fail(phase, f'barrier before {what} broke (another thread did not arrive)')


def _thread_main(N, t, cases, barrier, tally, record):
    ctx = tally.guarded('A', 'N.Context', lambda: N.Context(N.default_device()))
    record['ctx'] = ctx
    # phase A: first calls together
    for f in FAMILIES_A:
        _wait(barrier, tally, 'A', f.name)
        run_family(N, ctx, f, cases[t, f.name, 0], False, tally, 'A', 'first call')
    # phase B: different families at once
    for r in range(1, ROUNDS_B + 1):
        for s in range(len(FAMILIES_B)):
            f = FAMILIES_B[rotation(s, t)]
            _wait(barrier, tally, 'B', f'round {r} step {s}')
            run_family(N, ctx, f, cases[t, f.name, r], True, tally, 'B', f'round {r} step {s}')
    # phase C: what is thread-local stays thread-local
    _wait(barrier, tally, 'C', 'the refusal')

    def refusal():
        if t == 0:
            try:
                N.resize(np.zeros((8, 8), np.uint8), (16, 16), AREA, ctx=ctx)      # refused on the host, nothing is queued
                raised = False
            except N.VkxError:
                raised = True
            text = N.last_error()
            tally.check('C', raised and REFUSAL in text, f'the enlarging AREA resize: raised {raised}, last_error {text!r}')
        else:
            case = cases[t, ColorShift.name, ROUNDS_B + 1]
            run_family(N, ctx, ColorShift, case, False, tally, 'C', 'beside the refusal')
    tally.guarded('C', 'refusal', refusal)
    _wait(barrier, tally, 'C', 'reading last_error')          # thread 0 has been refused by now
    if t != 0:
        text = tally.guarded('C', 'last_error', N.last_error)
        tally.check('C', text is not None and REFUSAL not in text, f"another thread's refusal in last_error: {text!r}")
    record['last_error'] = tally.guarded('C', 'last_error', N.last_error)

    _wait(barrier, tally, 'C', 'resident mode')
    if t in (1, 2):
        barrier2 = record['pair_barrier']      # threads 1 and 2 alone: the call outside happens while thread 1 is inside

        def resident():
            case = cases[t, ColorShift.name, ROUNDS_B + 1]
            if t == 1:
                with N.resident(True):
                    _wait(barrier2, tally, 'C', 'the call inside N.resident')
                    got = N.color_shift_rgb(case['img'], case['delta'], ctx=ctx)
            else:
                _wait(barrier2, tally, 'C', 'the call outside N.resident')
                got = N.color_shift_rgb(case['img'], case['delta'], ctx=ctx)
            record['resident_kind'] = type(got).__name__
            want_kind = N.DevArray if t == 1 else np.ndarray
            tally.check('C', isinstance(got, want_kind) and same(_host(got), case['want'][0]) is None,
                        f'{type(got).__name__} {"inside" if t == 1 else "outside"} N.resident(True), or wrong pixels')
        tally.guarded('C', 'resident mode', resident)

    _wait(barrier, tally, 'C', 'default_ctx')
    first = tally.guarded('C', 'default_ctx', N.default_ctx)
    second = tally.guarded('C', 'default_ctx', N.default_ctx)
    tally.check('C', first is not None and first is second, 'N.default_ctx() gave another object on the second call')
    record['default_ctx'] = first
    _wait(barrier, tally, 'C', 'the end')
    if ctx is not None:
        tally.guarded('C', 'ctx.sync', ctx.sync)


def run_threads():
    """The whole scenario: ({phase: comparisons made}, declined poisson images, failures, records of phase C)"""
    from vkit_amd import _native as N
    cases = expectations()
    N.lib()
    barrier, pair = threading.Barrier(THREADS), threading.Barrier(2)
    tallies = [Tally(f'thread {t}') for t in range(THREADS)]
    records = [{'pair_barrier': pair} for _ in range(THREADS)]

    def main(t):
        try:
            _thread_main(N, t, cases, barrier, tallies[t], records[t])
        except Exception:
            tallies[t].fail('?', 'the thread ended early: ' + traceback.format_exc()[-1500:])
            barrier.abort()

    threads = [threading.Thread(target=main, args=(t,), name=f'vkx-thread-{t}') for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    top = Tally('main thread')
    ctxs = [r.get('default_ctx') for r in records]
    own = [r.get('ctx') for r in records]
    top.check('C', all(c is not None for c in ctxs) and len({id(c) for c in ctxs}) == THREADS
              and not {id(c) for c in ctxs} & {id(c) for c in own},
              'N.default_ctx() of four threads are not four distinct contexts')
    compared = {}
    for tl in tallies + [top]:
        for phase, n in tl.compared.items():
            compared[phase] = compared.get(phase, 0) + n
    failures = [f for tl in tallies + [top] for f in tl.failures]
    phase_c = {'last_error': [r.get('last_error') for r in records],
               'resident_kind': {str(t): records[t].get('resident_kind') for t in (1, 2)},
               'default_ctx_distinct': len({id(c) for c in ctxs if c is not None})}
    for c in own:
        if c is not None:
            c.close()
    return compared, sum(tl.declined for tl in tallies), failures, phase_c


SENTINEL = 'thread contexts child:'


def child_main():
    """what the child process runs: the scenario, then one report line"""
    import json
    import time
    t0 = time.perf_counter()
    compared, declined, failures, phase_c = run_threads()
    print(SENTINEL, json.dumps({'compared': compared, 'declined': declined, 'failures': failures[:40], 'n_failures': len(failures),
                                'phase_c': phase_c, 'seconds': round(time.perf_counter() - t0, 2)}))


# ---- two contexts on one thread ----------------------------------------------------------------------------------------------

def interleave(N, first, second, cases_first, cases_second, tally, tag):
    """every phase B family queued on `first`, then on `second`, with no synchronisation between the two beyond what a wrapper
    itself waits for; both synchronised once at the end; then every result compared.  Returns the results of `first`.
    (set_mask goes through the element layer, which has no ctx argument: both of its turns run on the thread's default context.)"""
    handles = []
    for f in FAMILIES_B:
        ha = tally.guarded('B', f'{f.name} {tag}', lambda: f.queue(N, first, cases_first[f.name], True))
        hb = tally.guarded('B', f'{f.name} {tag}', lambda: f.queue(N, second, cases_second[f.name], True)) if second else None
        handles.append((f, ha, hb))
    first.sync()
    if second:
        second.sync()
    results = {}
    for f, ha, hb in handles:
        for handle, cases, keep in ((ha, cases_first, True), (hb, cases_second, False)):
            if handle is None:
                continue
            got = tally.guarded('B', f'{f.name} {tag} collect', lambda: f.collect(N, handle))
            if got is not None:
                tally.compare('B', f, got, cases[f.name]['want'], tag)
                if keep:
                    results[f.name] = got
    return results
