"""The JPEG encoder of Image.to_file (reference image.py:351-359) on the CPU: tests/jpeg_encode_restate.py against the files
Pillow's libjpeg-turbo wrote (tests/golden/jpeg_encode.npz), whole file; the census of the block coder's events over the golden
cases; the header fields one by one; the C entry point declared, exported and bound."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import jpeg_encode_restate as E  # noqa: E402
import jpeg_restate as J  # noqa: E402
from jpeg_encode_cases import golden_cases  # noqa: E402


def test_restatement_equals_every_golden_file_and_meets_every_event(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jpeg_encode.npz'))
    assert str(z['libjpeg_turbo']).startswith('3.') and str(z['pillow'])
    census = dict.fromkeys(E.EVENTS, 0)
    n = 0
    for name, mat, q, want in golden_cases(golden_dir):
        got, events = E.encode(mat, q)
        assert got == want, (name, q, len(got), len(want))
        for key, count in events.items():
            census[key] += count
        n += 1
    assert n >= 150
    # coverage is a condition: every branch of the block coder, the stuffing included, is met by some case
    missing = [e for e in E.REQUIRED_EVENTS if not census[e]]
    assert not missing, (missing, census)


def test_goldens_cover_the_issue_space(golden_dir):
    cases = list(golden_cases(golden_dir))
    names = {name for name, *_ in cases}
    shapes = {tuple(int(v) for v in n.split('_')[0].split('x')[:2]) for n in names}
    assert shapes == {(1, 1), (1, 300), (300, 1), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 33), (97, 141), (256, 256)}
    assert {v % 16 for s in shapes for v in s} >= {0, 1, 7, 9, 15}
    assert {n.split('_')[0].split('x')[2] for n in names} == {'1', '3'}
    assert {n.split('_', 1)[1] for n in names} == {'random', 'gradient', 'saturated', 'asymmetric', 'constant', 'blocks8'}
    per_shape = {}
    for name, _mat, q, _want in cases:
        per_shape.setdefault(name.rsplit('x', 1)[0], set()).add(q)
    assert all(qs == {1, 10, 50, 75, 95, 100} for qs in per_shape.values()), per_shape
    # quality 75 (what Image.to_file writes) meets both modes
    assert {n.split('_')[0].split('x')[2] for n, _m, q, _w in cases if q == 75} == {'1', '3'}
    # 256 x 256 makes 1536 blocks: 12 rounds of the 128-entry scan the device runs over an image of up to 2048 blocks (the chunks
    # of its stream: 2 rounds)
    assert any(len(E.scan_blocks(mat, 75)) == 1536 for name, mat, q, _w in cases if name.startswith('256x256x3') and q == 75)
    # the channel order matters on the asymmetric case
    for name, mat, q, want in cases:
        if name == '97x141x3_asymmetric':
            assert E.encode_bytes(np.ascontiguousarray(mat[..., ::-1]), q) != want
            assert E.encode_bytes(np.ascontiguousarray(mat[..., ::-1]), q, bgr=True) == want


def test_dummy_blocks_follow_compress_data():
    """17 x 33 RGB: 3 x 5 luma blocks in 2 x 3 MCUs: the last MCU column misses its right blocks, the last MCU row its lower ones."""
    rng = np.random.default_rng(3)
    mat = rng.integers(0, 256, (17, 33, 3), dtype=np.uint8)
    blocks = E.scan_blocks(mat, 90)
    assert len(blocks) == 6 * 2 * 3 and [c for c, _ in blocks[:6]] == [0, 0, 0, 0, 1, 2]
    y = E.quantised_blocks(J._luma_plane(J.rgb_to_ycc(mat[..., 0], mat[..., 1], mat[..., 2])[0]), J.quant_tables(90)[0])
    assert y.shape[:2] == (3, 5)

    def mcu(my, mx):
        return [coef for _c, coef in blocks[6 * (my * 3 + mx):][:4]]

    y00, y01, y10, y11 = mcu(0, 2)                # the right column is missing
    assert (y00 == y[0, 4]).all() and (y10 == y[1, 4]).all()
    assert y01[0] == y00[0] and not y01[1:].any() and y11[0] == y10[0] and not y11[1:].any()
    y00, y01, y10, y11 = mcu(1, 0)                # the lower row is missing: both take the DC of Y01
    assert (y00 == y[2, 0]).all() and (y01 == y[2, 1]).all()
    assert y10[0] == y01[0] == y11[0] and not y10[1:].any() and not y11[1:].any()
    y00, y01, y10, y11 = mcu(1, 2)                # both: Y01 is a dummy itself
    assert (y00 == y[2, 4]).all() and y01[0] == y10[0] == y11[0] == y00[0]
    assert not y01[1:].any() and not y10[1:].any() and not y11[1:].any()


def test_header_fields():
    for cn, h, w, q in ((3, 97, 141, 75), (1, 300, 1, 10), (3, 1, 1, 100), (1, 32768, 32768, 0)):
        segs = E.header_segments(h, w, cn, q)
        names = [name for name, _ in segs]
        want = ['SOI', 'APP0', 'DQT0'] + (['DQT1'] if cn == 3 else []) + ['SOF0', 'DHT_DC0', 'DHT_AC0']
        want += (['DHT_DC1', 'DHT_AC1'] if cn == 3 else []) + ['SOS']
        assert names == want
        seg = dict(segs)
        assert seg['SOI'] == b'\xff\xd8'
        for name, data in segs[1:]:
            assert data[0] == 0xFF and int.from_bytes(data[2:4], 'big') == len(data) - 2, name
        # JFIF 1.1, unit 0, density 1 x 1, no thumbnail
        assert seg['APP0'] == b'\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
        luma, chroma = J.quant_tables(q)
        assert len(seg['DQT0']) == 69 and seg['DQT0'][4] == 0 and list(seg['DQT0'][5:]) == [int(v) for v in luma[E.ZIGZAG]]
        if cn == 3:
            assert len(seg['DQT1']) == 69 and seg['DQT1'][4] == 1 and list(seg['DQT1'][5:]) == [int(v) for v in chroma[E.ZIGZAG]]
        sof = seg['SOF0']
        assert sof[1] == 0xC0 and sof[4] == 8 and int.from_bytes(sof[5:7], 'big') == h and int.from_bytes(sof[7:9], 'big') == w
        assert sof[9] == cn
        comps = [tuple(sof[10 + 3 * c:13 + 3 * c]) for c in range(cn)]
        assert comps == ([(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] if cn == 3 else [(1, 0x11, 0)])
        # the DHT segments are the Annex K tables: 31 and 181 bytes after the marker
        for name, table, tc_th in (('DHT_DC0', E.DC_LUMA, 0x00), ('DHT_AC0', E.AC_LUMA, 0x10), ('DHT_DC1', E.DC_CHROMA, 0x01),
                                   ('DHT_AC1', E.AC_CHROMA, 0x11)):
            if name not in seg:
                continue
            data = seg[name]
            assert data[1] == 0xC4 and len(data) - 2 == (31 if 'DC' in name else 181) and data[4] == tc_th
            assert tuple(data[5:21]) == table[0] and tuple(data[21:]) == table[1] and sum(table[0]) == len(table[1])
        sos = seg['SOS']
        assert sos[1] == 0xDA and sos[4] == cn and sos[-3:] == b'\x00\x3f\x00'
        assert [tuple(sos[5 + 2 * c:7 + 2 * c]) for c in range(cn)] == [(1, 0x00), (2, 0x11), (3, 0x11)][:cn]
        assert len(E.header(h, w, cn, q)) == (623 if cn == 3 else 2 + 18 + 69 + 13 + 33 + 183 + 10)


def test_huffman_codes_are_prefix_free_and_complete_enough():
    for name, codes in E.CODES.items():
        words = sorted(format(code, f'0{length}b') for code, length in codes.values())
        assert all(not b.startswith(a) for a, b in zip(words, words[1:])), name
        assert len(codes) == (12 if name.startswith('dc') else 162)
        assert max(length for _code, length in codes.values()) == (16 if name.startswith('ac') else (9 if name == 'dc0' else 11))
    # the longest a block can get: the bound the device's unstuffed stream is sized by
    longest_dc = max(length + size for t in ('dc0', 'dc1') for size, (_c, length) in E.CODES[t].items())
    longest_ac = max(length + (sym & 15) for t in ('ac0', 'ac1') for sym, (_c, length) in E.CODES[t].items())
    # (luma: a 9-bit code and 11 magnitude bits; the chroma table's category 11 has an 11-bit code)
    assert longest_dc == 11 + 11 and longest_ac == 16 + 10 and longest_dc + 63 * longest_ac <= 208 * 8
    # a lane's share: three ZRL, a code, the magnitude bits
    assert 3 * max(E.CODES[t][0xF0][1] for t in ('ac0', 'ac1')) + longest_ac <= 59 and longest_dc <= 59


def test_stuffing_and_padding_on_crafted_streams():
    census = dict.fromkeys(E.EVENTS, 0)
    # an all-zero grey block at DC 0: DC category 0 (code 00) and EOB (1010): 6 bits, padded with two 1-bits
    assert E.encode_scan([(0, np.zeros(64, np.int64))], census) == bytes([0b00101011])
    assert census['zero_ac'] == 1 and census['dc_cat0'] == 1 and census['no_padding'] == 0
    # a coefficient at zigzag 63 after 62 zeros: three ZRL, no EOB
    coef = np.zeros(64, np.int64)
    coef[63] = 1
    census = dict.fromkeys(E.EVENTS, 0)
    E.encode_scan([(0, coef)], census)
    assert census['zrl3'] == 1 and census['no_eob'] == 1 and census['zrl1'] == census['zrl2'] == 0


def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, 'include', 'vkx.h')).read()
    assert re.search(r'\bint\s+vkx_jpeg_encode_u8_dev\s*\(', text)
    assert 'image.py:351-359' in text
    from vkit_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), 'vkx_jpeg_encode_u8_dev')
    assert 'vkx_jpeg_encode_u8_dev' in _native.EXPORTED_SYMBOLS and callable(_native.jpeg_encode)
    assert ctypes.sizeof(_native.VkxJpegImage) == 24
    from vkit_amd.element import Image, encode_jpeg_images
    assert callable(encode_jpeg_images) and all(hasattr(Image, m) for m in ('to_file', 'to_pil_image', 'to_jpeg_bytes'))


def test_import_stays_light():
    import subprocess
    code = 'import sys, vkit_amd, vkit_amd.element; assert "torch" not in sys.modules and "PIL" not in sys.modules'
    subprocess.run([sys.executable, '-c', code], cwd=ROOT, check=True)
