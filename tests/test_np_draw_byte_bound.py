"""The bound the byte-parked draw pass rests on (csrc/nprand.hip, np_parks_as_bytes / EmitI16B8), without a GPU.

  bound   a fast accept of layer idx has rabs < ki[idx], so |x| <= (ki[idx] - 1) * wi[idx]: for all 256 layers of the tables the
          library carries (csrc/np_ziggurat.h, numpy's) that is at most r = 3.6541528853610088, hence |rint(scale x + loc)| <= r |scale| + |loc|
  rule    the library's own statement of the selection (vkx_np_parks_as_bytes) on either side of r |scale| + |loc| = 127 and on it,
          with loc = 0 (std 34.75 / 34.76) and with locations of both signs"""
import math
import os
import re
import struct

import pytest

from vkit_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 3.6541528853610088


def _table(text, name):
    body = re.search(name + r'\[256\] = \{(.*?)\};', text, re.S).group(1)
    vals = [int(v, 16) for v in re.findall(r'0x([0-9a-fA-F]+)ull', body)]
    assert len(vals) == 256
    return vals


def test_every_fast_accept_is_at_most_r():
    with open(os.path.join(ROOT, 'vkit_amd', 'csrc', 'np_ziggurat.h')) as fin:
        text = fin.read()
    ki = _table(text, 'kNpZigK')
    wi = [struct.unpack('<d', struct.pack('<Q', b))[0] for b in _table(text, 'kNpZigW')]
    worst = 0.0
    for idx in range(256):
        assert 0 <= ki[idx] < 1 << 52 and wi[idx] > 0.0
        if ki[idx] == 0:
            continue                    # no rabs is below 0: the layer has no fast accept
        x = float(ki[idx] - 1) * wi[idx]          # ki - 1 < 2^52 is exact in float64; one rounding, as in the kernel
        assert x <= R, idx
        worst = max(worst, x)
    assert worst > 3.6           # the bound is the base layer's, and tight


def _parks(scale, loc):
    return N.lib().vkx_np_parks_as_bytes(float(scale), float(loc))


@pytest.mark.parametrize('loc', [0.0, 20.0, -20.0, 90.5, -126.0])
def test_rule_on_either_side_of_127(loc):
    room = 127.0 - abs(loc)
    at = room / R
    # the rule's own float64 expression, evaluated here: which side a given scale falls on is what the library must say too
    for scale in (at * (1 - 1e-9), at, at * (1 + 1e-9), math.nextafter(at, 0.0), math.nextafter(at, math.inf)):
        for s in (scale, -scale):
            want = 1 if R * abs(s) + abs(loc) <= 127.0 else 0
            assert _parks(s, loc) == want, (s, loc)
    assert _parks(at * (1 - 1e-9), loc) == 1 and _parks(at * (1 + 1e-9), loc) == 0


def test_rule_at_the_deviations_of_the_issue():
    assert _parks(34.75, 0.0) == 1 and _parks(34.76, 0.0) == 0
    assert _parks(10.0, 0.0) == 1 and _parks(10.0, 20.0) == 1 and _parks(10.0, -20.0) == 1
    assert _parks(10.0, 90.5) == 0 and _parks(10.0, -90.5) == 0
    assert _parks(60.0, 0.0) == 0 and _parks(0.0, 127.0) == 1 and _parks(0.0, -127.5) == 0
    assert _parks(float('nan'), 0.0) == 0 and _parks(float('inf'), 0.0) == 0
