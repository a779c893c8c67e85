"""The batch collate of vkit_amd/torch_bridge.py restated in numpy (bfloat16: torch on the CPU), from the contract of
include/vkx.h alone:

    out = (float32(x) - m_c) * s_c,   m_c = float32(255 mean_c),   s_c = float32(1 / (255 std_c))

m and s each worked out in float64 and rounded once; one float32 subtraction, one float32 multiplication, and for the 16-bit
types one more rounding to nearest even.  uint8 is the plain stack / transpose.  Labels are stacked as they are.
"""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
DTYPES = ('uint8', 'float32', 'float16', 'bfloat16')
# (mean, std) that take the arithmetic to its edges, by what they reach over every byte value in every channel:
EDGE_CONSTANTS = {
    'f16_subnormal': ((0.5, 0.5, 0.5), (40.0, -300.0, 2000.0)),              # float16 subnormals, a negative scale
    'f16_infinite': ((0.0, 0.3, 1.0), (1e-4, -2e-5, 1e-6)),                  # float16 infinities and zeros
    'subnormal_scale': ((0.5, 0.5, 0.5), (1e36, -1e37, 3e37)),               # float32 / bfloat16 subnormals; float16 zeros of both signs
    'f32_infinite': ((0.0, 0.5, 1.0), (1e-39, -1.2e-39, 5e-40)),             # float32 / bfloat16 infinities of both signs beside finite values
}
# the classes (keys of ``classes``) each set is there for, by output dtype: a test asserts them present in the restatement's output
EDGE_REACHES = {
    'f16_subnormal': {'float16': ('subnormal',)},
    # (f16_infinite: every infinity is negative -- only channel 2, (x - 255) * 3921.6 <= 0, leaves float16; |channel 0| <= 10 000, |channel 1| <= 35 000)
    'f16_infinite': {'float16': ('-inf', 'zero'), 'float32': ('zero',), 'bfloat16': ('zero',)},
    'subnormal_scale': {'float32': ('subnormal',), 'bfloat16': ('subnormal',), 'float16': ('zero', '-zero')},
    'f32_infinite': {'float32': ('inf', '-inf', 'finite'), 'bfloat16': ('inf', '-inf', 'finite'), 'float16': ('inf', '-inf')},
}


def edge_image():
    """The (16, 16, 3) image whose 768 bytes hold every byte value in every channel."""
    return np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(16, 16, 3)


def constants(mean=MEAN, std=STD):
    m = np.array([np.float32(np.float64(255.0) * np.float64(v)) for v in mean], np.float32)
    s = np.array([np.float32(np.float64(1.0) / (np.float64(255.0) * np.float64(v))) for v in std], np.float32)
    return m, s


def collate_images(images, dtype='float32', mean=MEAN, std=STD, channels_first=True):
    """uint8 (h, w, 3) arrays -> the batch: a numpy array, or a torch CPU tensor for bfloat16."""
    x = np.stack([np.asarray(i) for i in images])
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[3] == 3
    if dtype == 'uint8':
        out = x
    else:
        m, s = constants(mean, std)
        diff = x.astype(np.float32) - m                 # float32 - float32: one rounding
        assert diff.dtype == np.float32
        with np.errstate(over='ignore', under='ignore'):
            out = diff * s                              # one rounding
        assert out.dtype == np.float32
    if channels_first:
        out = out.transpose(0, 3, 1, 2)
    out = np.ascontiguousarray(out)
    if dtype == 'float16':
        with np.errstate(over='ignore', under='ignore'):
            return out.astype(np.float16)               # round to nearest even
    if dtype == 'bfloat16':
        import torch
        return torch.from_numpy(out).to(torch.bfloat16)
    return out


def collate_planes(planes):
    return np.stack([np.asarray(p) for p in planes])


def bits(a):
    """The bit pattern of a batch (numpy array or torch tensor, any of the four dtypes) as a numpy integer array."""
    if not isinstance(a, np.ndarray):
        import torch
        a = a.detach().cpu().contiguous()
        if a.dtype == torch.bfloat16:
            return a.view(torch.int16).numpy()
        a = a.numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def classes(a):
    """How many elements of a float batch (float32, float16 or bfloat16; numpy array or torch tensor) are subnormal, infinite, NaN and
    zero, by sign where it matters: a dict of counts read off the bit patterns."""
    name = str(a.dtype).replace('torch.', '')
    sign, exponent, mantissa = {'float32': (0x80000000, 0x7F800000, 0x007FFFFF), 'float16': (0x8000, 0x7C00, 0x03FF),
                                'bfloat16': (0x8000, 0x7F80, 0x007F)}[name]
    b = bits(a)
    b = b.astype(np.int64) & (sign | exponent | mantissa)
    e, f, negative = b & exponent, b & mantissa, (b & sign) != 0
    top, zero = e == exponent, (e == 0) & (f == 0)
    return {'subnormal': int(((e == 0) & (f != 0)).sum()), 'nan': int((top & (f != 0)).sum()),
            'inf': int((top & (f == 0) & ~negative).sum()), '-inf': int((top & (f == 0) & negative).sum()),
            'zero': int((zero & ~negative).sum()), '-zero': int((zero & negative).sum()),
            'finite': int((~top).sum()), 'size': int(b.size)}
