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
        out = diff * s                                  # one rounding
        assert out.dtype == np.float32
    if channels_first:
        out = out.transpose(0, 3, 1, 2)
    out = np.ascontiguousarray(out)
    if dtype == 'float16':
        return out.astype(np.float16)                   # round to nearest even
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
