"""A numpy / Python restatement of libjpeg-turbo's baseline JPEG *encoder* as Pillow drives it with its defaults
(``Image.save(f, format='JPEG', quality=q)``: JFIF 1.1, 4:2:0 for RGB, one component for grey, the Annex K Huffman tables, no
restart markers), down to the byte.

Test infrastructure only: the device encoder (vkit_amd/csrc/jpeg_encode.hip) is pinned against this, and this is pinned against
the library itself (tests/golden/jpeg_encode.npz, and a live Pillow where one is installed).  The lossy half -- colour
conversion, h2v2 downsampling, forward DCT, quantisation -- is tests/jpeg_restate.py's; this file adds the lossless half:

* the MCU interleave with the dummy blocks of ``compress_data`` (jccoefct.c): a block right of a component's last block column
  inside an MCU has zero AC and the DC of the block before it; a block row below the last one has zero AC and the DC of the
  last block of the MCU's row above it;
* the Annex K tables and the block coder of ``encode_one_block`` (jchuff.c);
* the final padding with 1-bits (``flush_bits``) and the 0x00 after every 0xFF of the scan;
* the headers, in the order and with the lengths libjpeg writes them.

``encode`` also returns a census of the coder's events over the stream, so that a set of cases can be shown to reach every
branch (EVENTS).
"""
import numpy as np

import jpeg_restate as J

# jpeg_natural_order: zigzag position -> natural (row-major) index
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.3: (number of codes of each length 1 .. 16, the symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))

# the census: every event the block coder, the padding and the stuffing can meet
EVENTS = ('zrl1', 'zrl2', 'zrl3', 'no_eob', 'zero_ac', 'dc_cat0', 'dc_cat11', 'ac_size10', 'stuffed', 'stuffed_padding',
          'no_padding')
# ... the last two depend on where the stream happens to end: a set of cases need not hold them
REQUIRED_EVENTS = EVENTS[:-2]


def huffman_codes(table):
    """symbol -> (code, length) of a (bits, values) table: the canonical codes of Annex C."""
    bits, values = table
    assert sum(bits) == len(values)
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


CODES = {name: huffman_codes(t) for name, t in (('dc0', DC_LUMA), ('ac0', AC_LUMA), ('dc1', DC_CHROMA), ('ac1', AC_CHROMA))}


def quantised_blocks(plane, qtable):
    """A padded sample plane (multiples of 8 on both sides) -> the quantised coefficients [bh, bw, 64] in zigzag order."""
    blk = J._blocks(np.asarray(plane, np.int64) - 128)
    coef = J._fdct_pass(J._fdct_pass(blk, False).swapaxes(-1, -2), True).swapaxes(-1, -2)
    div = 8 * qtable.reshape(8, 8)
    mag = (np.abs(coef) + (div >> 1)) // div
    q = np.where(coef < 0, -mag, mag)
    return q.reshape(q.shape[0], q.shape[1], 64)[..., ZIGZAG]


def scan_blocks(mat, quality, bgr=False):
    """The blocks of the scan in the order the entropy coder meets them: ``[(component, coef[64] in zigzag order)]``, the
    dummy blocks of ``compress_data`` included.  Grey: one component, its blocks row-major.  Colour: per 16 x 16 MCU
    Y00 Y01 Y10 Y11 Cb Cr, the MCUs row-major."""
    mat = np.asarray(mat)
    assert mat.dtype == np.uint8 and 0 <= quality <= 100
    luma_q, chroma_q = J.quant_tables(quality)
    if mat.ndim == 2:
        y = quantised_blocks(J._luma_plane(mat.astype(np.int64)), luma_q)
        return [(0, y[by, bx]) for by in range(y.shape[0]) for bx in range(y.shape[1])]
    assert mat.ndim == 3 and mat.shape[2] == 3
    r, g, b = (mat[..., 2], mat[..., 1], mat[..., 0]) if bgr else (mat[..., 0], mat[..., 1], mat[..., 2])
    yy, cb, cr = J.rgb_to_ycc(r, g, b)
    y = quantised_blocks(J._luma_plane(yy), luma_q)
    cb = quantised_blocks(J._chroma_plane(cb), chroma_q)
    cr = quantised_blocks(J._chroma_plane(cr), chroma_q)
    ybh, ybw = y.shape[:2]
    mcus_y, mcus_x = cb.shape[:2]
    assert (mcus_y, mcus_x) == ((ybh + 1) // 2, (ybw + 1) // 2) == cr.shape[:2]
    out = []
    for my in range(mcus_y):
        for mx in range(mcus_x):
            first = len(out)
            for yi in range(2):
                for xi in range(2):
                    by, bx = 2 * my + yi, 2 * mx + xi
                    if by < ybh and bx < ybw:
                        out.append((0, y[by, bx]))
                        continue
                    dummy = np.zeros(64, np.int64)
                    # a missing column: the DC of the block before it; a missing row: the DC of the last block of the row above
                    dummy[0] = out[-1][1][0] if by < ybh else out[first + 1][1][0]
                    out.append((0, dummy))
            out.append((1, cb[my, mx]))
            out.append((2, cr[my, mx]))
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.n += length


def _bit_length(v):
    return int(v).bit_length()


def encode_scan(blocks, census):
    """The entropy-coded segment of ``scan_blocks``' list, padded and stuffed."""
    bits = _Bits()
    last_dc = {}
    for comp, coef in blocks:
        tab = 0 if comp == 0 else 1
        dc, ac = CODES[f'dc{tab}'], CODES[f'ac{tab}']
        diff = int(coef[0]) - last_dc.get(comp, 0)
        last_dc[comp] = int(coef[0])
        size = _bit_length(abs(diff))
        assert size <= 11
        census['dc_cat0'] += size == 0
        census['dc_cat11'] += size == 11
        bits.put(*dc[size])
        if size:
            bits.put((diff if diff >= 0 else diff - 1) & ((1 << size) - 1), size)
        run = 0
        nonzero = False
        for k in range(1, 64):
            v = int(coef[k])
            if v == 0:
                run += 1
                continue
            nonzero = True
            if run >> 4:
                census[f'zrl{run >> 4}'] += 1
            for _ in range(run >> 4):
                bits.put(*ac[0xF0])
            size = _bit_length(abs(v))
            assert 1 <= size <= 10
            census['ac_size10'] += size == 10
            bits.put(*ac[((run & 15) << 4) | size])
            bits.put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)
            run = 0
        if run:
            bits.put(*ac[0x00])
        else:
            census['no_eob'] += 1
        census['zero_ac'] += not nonzero
    pad = -bits.n % 8
    census['no_padding'] += pad == 0
    if pad:
        bits.put((1 << pad) - 1, pad)
    raw = bits.acc.to_bytes(bits.n // 8, 'big') if bits.n else b''
    census['stuffed'] += raw.count(b'\xff')
    census['stuffed_padding'] += bool(pad) and raw[-1:] == b'\xff'
    return raw.replace(b'\xff', b'\xff\x00')


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def header_segments(h, w, cn, quality):
    """The segments before the scan, in order, as ``[(name, bytes)]``: SOI, APP0, DQT per table, SOF0, DHT per table, SOS."""
    luma_q, chroma_q = J.quant_tables(quality)
    segs = [('SOI', b'\xff\xd8'),
            ('APP0', _segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])))]
    for i, q in enumerate((luma_q, chroma_q)[:1 if cn == 1 else 2]):
        segs.append((f'DQT{i}', _segment(0xDB, bytes([i]) + bytes(int(v) for v in q[ZIGZAG]))))
    comps = [(1, 0x11, 0)] if cn == 1 else [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
    sof = bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([len(comps)])
    for cid, sampling, tq in comps:
        sof += bytes([cid, sampling, tq])
    segs.append(('SOF0', _segment(0xC0, sof)))
    tables = [('DHT_DC0', 0x00, DC_LUMA), ('DHT_AC0', 0x10, AC_LUMA)]
    if cn == 3:
        tables += [('DHT_DC1', 0x01, DC_CHROMA), ('DHT_AC1', 0x11, AC_CHROMA)]
    for name, tc_th, (bits, values) in tables:
        segs.append((name, _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(values))))
    sos = bytes([len(comps)])
    for cid, _sampling, tq in comps:
        sos += bytes([cid, tq << 4 | tq])
    segs.append(('SOS', _segment(0xDA, sos + bytes([0, 63, 0]))))
    return segs


def header(h, w, cn, quality):
    return b''.join(s for _name, s in header_segments(h, w, cn, quality))


def encode(mat, quality, bgr=False):
    """``(file bytes, census)`` of ``PIL.Image.fromarray(mat).save(f, 'JPEG', quality=quality)`` for uint8 H x W (mode L) or
    H x W x 3 (mode RGB; ``bgr``: channel 2 carries the red weight, as ``cv.imencode`` reads a mat)."""
    mat = np.asarray(mat)
    h, w = mat.shape[:2]
    census = dict.fromkeys(EVENTS, 0)
    scan = encode_scan(scan_blocks(mat, quality, bgr), census)
    return header(h, w, 1 if mat.ndim == 2 else 3, quality) + scan + b'\xff\xd9', census


def encode_bytes(mat, quality, bgr=False):
    return encode(mat, quality, bgr)[0]


def split_header(data):
    """A JPEG file as ``(header up to and including SOS, scan, EOI)``."""
    data = bytes(data)
    at = 2
    assert data[:2] == b'\xff\xd8'
    while True:
        assert data[at] == 0xFF
        length = int.from_bytes(data[at + 2:at + 4], 'big')
        marker = data[at + 1]
        at += 2 + length
        if marker == 0xDA:
            break
    return data[:at], data[at:-2], data[-2:]


def pillow_encode(mat, quality):
    """The same file through Pillow (mode L or RGB: channel 0 is red)."""
    import io

    from PIL import Image as PILImage
    mat = np.ascontiguousarray(mat)
    buf = io.BytesIO()
    PILImage.fromarray(mat, 'L' if mat.ndim == 2 else 'RGB').save(buf, format='JPEG', quality=int(quality))
    return buf.getvalue()
