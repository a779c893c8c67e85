"""A numpy restatement of libjpeg-turbo's baseline JPEG round trip, ``decode(encode(mat, quality))``, as the reference drives it
through ``cv.imencode('.jpeg', mat, [IMWRITE_JPEG_QUALITY, q])`` / ``cv.imdecode`` (photometric/effect.py:41-42).

Test infrastructure only: the device kernel (vkit_amd/csrc/jpeg.hip) is pinned against this, and this is pinned against the
library itself (tests/golden/jpeg_roundtrip.npz, and Pillow where it is installed).  Entropy coding is lossless, so the round
trip is: RGB->YCbCr, h2v2 downsampling, 8x8 accurate integer forward DCT, quantise, dequantise, accurate integer inverse DCT,
h2v2 fancy upsampling, YCbCr->RGB.  A 3-channel mat is BGR to cv2: channel 2 carries the R weight, and the decoder writes
back in the same order.  A 2-D mat is a one-component (grayscale) JPEG.
"""
import numpy as np

# Annex K tables, natural (row-major) order
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)


def quant_tables(quality):
    """(luma, chroma) 64-entry tables of ``jpeg_set_quality(quality, force_baseline=TRUE)``, natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((std * scale + 50) // 100, 1, 255) for std in (STD_LUMA, STD_CHROMA))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


C_0_298, C_0_390, C_0_541, C_0_765 = 2446, 3196, 4433, 6270
C_0_899, C_1_175, C_1_501, C_1_847 = 7373, 9633, 12299, 15137
C_1_961, C_2_053, C_2_562, C_3_072 = 16069, 16819, 20995, 25172


def _fdct_pass(d, last):
    """One pass of the accurate integer forward DCT along the last axis of ``d`` (..., 8)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13 = t0 + t3, t0 - t3
    t11, t12 = t1 + t2, t1 - t2
    out = np.empty_like(d)
    sh = 13 + 2 if last else 13 - 2
    if last:
        out[..., 0] = _descale(t10 + t11, 2)
        out[..., 4] = _descale(t10 - t11, 2)
    else:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    z1 = (t12 + t13) * C_0_541
    out[..., 2] = _descale(z1 + t13 * C_0_765, sh)
    out[..., 6] = _descale(z1 - t12 * C_1_847, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C_1_175
    t4, t5, t6, t7 = t4 * C_0_298, t5 * C_2_053, t6 * C_3_072, t7 * C_1_501
    z1, z2, z3, z4 = -z1 * C_0_899, -z2 * C_2_562, -z3 * C_1_961 + z5, -z4 * C_0_390 + z5
    out[..., 7] = _descale(t4 + z1 + z3, sh)
    out[..., 5] = _descale(t5 + z2 + z4, sh)
    out[..., 3] = _descale(t6 + z2 + z3, sh)
    out[..., 1] = _descale(t7 + z1 + z4, sh)
    return out


def _idct_pass(d, last):
    """One pass of the accurate integer inverse DCT along the last axis of ``d`` (..., 8)."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * C_0_541
    t2 = z1 - z3 * C_1_847
    t3 = z1 + z2 * C_0_765
    t0 = (d[..., 0] + d[..., 4]) << 13
    t1 = (d[..., 0] - d[..., 4]) << 13
    t10, t13 = t0 + t3, t0 - t3
    t11, t12 = t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C_1_175
    t0, t1, t2, t3 = t0 * C_0_298, t1 * C_2_053, t2 * C_3_072, t3 * C_1_501
    z1, z2, z3, z4 = -z1 * C_0_899, -z2 * C_2_562, -z3 * C_1_961 + z5, -z4 * C_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    sh = 13 + 2 + 3 if last else 13 - 2
    out = np.empty_like(d)
    out[..., 0] = _descale(t10 + t3, sh)
    out[..., 7] = _descale(t10 - t3, sh)
    out[..., 1] = _descale(t11 + t2, sh)
    out[..., 6] = _descale(t11 - t2, sh)
    out[..., 2] = _descale(t12 + t1, sh)
    out[..., 5] = _descale(t12 - t1, sh)
    out[..., 3] = _descale(t13 + t0, sh)
    out[..., 4] = _descale(t13 - t0, sh)
    return out


def _idct_range_limit():
    """The post-IDCT sample table indexed by ``value & RANGE_MASK`` (1023): clamp(v + 128) on [-512, 512), wrapping beyond."""
    v = np.arange(1024)
    v = np.where(v >= 512, v - 1024, v)
    return np.clip(v + 128, 0, 255)


_RANGE_LIMIT = _idct_range_limit()


def _blocks(plane):
    ph, pw = plane.shape
    return plane.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(blocks):
    bh, bw = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def plane_roundtrip(plane, qtable):
    """Padded int plane (multiples of 8 on both sides) -> FDCT -> quantise -> dequantise -> IDCT -> uint8 samples."""
    blk = _blocks(plane.astype(np.int64) - 128)
    coef = _fdct_pass(_fdct_pass(blk, False).swapaxes(-1, -2), True).swapaxes(-1, -2)
    q = qtable.reshape(8, 8)
    div = 8 * q
    mag = (np.abs(coef) + (div >> 1)) // div
    deq = np.where(coef < 0, -mag, mag) * q
    ws = _idct_pass(deq.swapaxes(-1, -2), False).swapaxes(-1, -2)     # pass 1: columns
    out = _idct_pass(ws, True)                                        # pass 2: rows
    return _unblocks(_RANGE_LIMIT[out & 1023]).astype(np.uint8)


def _pad(n, m):
    return (n + m - 1) // m * m


# encoder colour conversion, 16-bit fixed point
def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(r, g, b):
    r, g, b = (np.asarray(c, np.int64) for c in (r, g, b))
    half = 1 << 15
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + half - 1) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + half - 1) >> 16
    return y, cb, cr


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (np.asarray(c, np.int64) for c in (y, cb, cr))
    half = 1 << 15
    x_cb, x_cr = cb - 128, cr - 128
    r = y + ((_fix(1.40200) * x_cr + half) >> 16)
    g = y + ((-_fix(0.34414) * x_cb + half - _fix(0.71414) * x_cr) >> 16)
    b = y + ((_fix(1.77200) * x_cb + half) >> 16)
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b))


def _luma_plane(y):
    """Edge replication to whole 8x8 blocks: columns on the right, rows at the bottom."""
    h, w = y.shape
    rows = np.minimum(np.arange(_pad(h, 8)), h - 1)
    cols = np.minimum(np.arange(_pad(w, 8)), w - 1)
    return y[rows][:, cols]


def _chroma_plane(c):
    """h2v2 downsampling to whole 8x8 blocks of the half-size component: the right edge replicated by input columns before
    the 2x2 sums, the bottom edge by repeating the last downsampled row; the rounding bias alternates 1, 2 along a row."""
    h, w = c.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    cy = np.minimum(np.arange(_pad(dh, 8)), dh - 1)
    cx = np.arange(_pad(dw, 8))
    r0, r1 = 2 * cy, np.minimum(2 * cy + 1, h - 1)
    c0, c1 = np.minimum(2 * cx, w - 1), np.minimum(2 * cx + 1, w - 1)
    s = c[r0][:, c0] + c[r0][:, c1] + c[r1][:, c0] + c[r1][:, c1]
    return (s + 1 + (cx & 1)) >> 2


def fancy_upsample(c, h, w):
    """h2v2 'fancy' (triangle) upsampling of the decoded half-size plane ``c`` to h x w: 3:1 weights in both directions,
    +8 / +7 rounding on even / odd output columns, neighbours clamped at the downsampled size (not the padded one).
    A component at most 2 samples wide is replicated instead (the library's fancy upsampler needs 3)."""
    dh, dw = (h + 1) // 2, (w + 1) // 2
    c = c[:dh, :dw].astype(np.int64)
    if dw <= 2:         # the library skips fancy upsampling of a component this narrow: plain 2x2 replication
        return c[np.arange(h) >> 1][:, np.arange(w) >> 1]
    y = np.arange(h)
    cy = y >> 1
    ny = np.clip(np.where(y & 1, cy + 1, cy - 1), 0, dh - 1)
    colsum = 3 * c[cy] + c[ny]                         # h x dw
    x = np.arange(w)
    cx = x >> 1
    nx = np.clip(np.where(x & 1, cx + 1, cx - 1), 0, dw - 1)
    return (3 * colsum[:, cx] + colsum[:, nx] + 8 - (x & 1)) >> 4


def jpeg_roundtrip(mat, quality):
    """``cv.imdecode(cv.imencode('.jpeg', mat, [IMWRITE_JPEG_QUALITY, quality]))`` for uint8 H x W (grayscale) or
    H x W x 3 (BGR to the codec) mats."""
    mat = np.asarray(mat)
    assert mat.dtype == np.uint8 and 0 <= quality <= 100
    luma_q, chroma_q = quant_tables(quality)
    if mat.ndim == 2:
        h, w = mat.shape
        return plane_roundtrip(_luma_plane(mat), luma_q)[:h, :w]
    assert mat.ndim == 3 and mat.shape[2] == 3
    h, w = mat.shape[:2]
    y, cb, cr = rgb_to_ycc(mat[..., 2], mat[..., 1], mat[..., 0])
    y_dec = plane_roundtrip(_luma_plane(y), luma_q)[:h, :w]
    cb_dec = fancy_upsample(plane_roundtrip(_chroma_plane(cb), chroma_q), h, w)
    cr_dec = fancy_upsample(plane_roundtrip(_chroma_plane(cr), chroma_q), h, w)
    r, g, b = ycc_to_rgb(y_dec, cb_dec, cr_dec)
    return np.stack([b, g, r], axis=-1)


def pillow_roundtrip(mat, quality):
    """The same round trip through Pillow's libjpeg-turbo (default 4:2:0, baseline tables, islow DCT, fancy upsampling)."""
    import io

    from PIL import Image as PILImage
    mat = np.asarray(mat)
    buf = io.BytesIO()
    if mat.ndim == 2:
        PILImage.fromarray(mat, 'L').save(buf, 'JPEG', quality=int(quality))
        return np.asarray(PILImage.open(io.BytesIO(buf.getvalue())).convert('L')).copy()
    PILImage.fromarray(np.ascontiguousarray(mat[..., ::-1]), 'RGB').save(buf, 'JPEG', quality=int(quality))
    out = np.asarray(PILImage.open(io.BytesIO(buf.getvalue())).convert('RGB'))
    return np.ascontiguousarray(out[..., ::-1])
