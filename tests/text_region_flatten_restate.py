"""numpy-plus-oracle restatement of the pixel half of PageTextRegionStep (reference: pipeline/text_detection/
page_text_region.py:560-656, :109-166, :732-856) for the tests of csrc/region_flatten.hip: the four operations on plain
arrays, one region at a time, with cv.warpAffine and cv.resize taken from the oracle."""
import math

import numpy as np

import oracle as O


def rotate_matrix(angle, shape):
    """RotateState of the reference (mechanism/distortion/geometric/affine.py): float32 forward matrix and dsize (w, h)"""
    height, width = shape
    rad = math.radians(angle % 360)
    sin, cos = math.sin, math.cos
    if rad <= math.pi / 2:
        shift_x, shift_y = height * sin(rad), 0
        dst_width, dst_height = height * sin(rad) + width * cos(rad), height * cos(rad) + width * sin(rad)
    elif rad <= math.pi:
        local = rad - math.pi / 2
        shift_x, shift_y = width * sin(local) + height * cos(local), height * sin(local)
        dst_width, dst_height = shift_x, shift_y + width * cos(local)
    elif rad < math.pi * 3 / 2:
        local = rad - math.pi
        shift_x, shift_y = width * cos(local), width * sin(local) + height * cos(local)
        dst_width, dst_height = shift_x + height * sin(local), shift_y
    else:
        local = rad - math.pi * 3 / 2
        shift_x, shift_y = 0, width * cos(local)
        dst_width, dst_height = width * sin(local) + height * cos(local), shift_y + height * sin(local)
    mat = np.asarray([(cos(rad), -sin(rad), math.ceil(shift_x)), (sin(rad), cos(rad), math.ceil(shift_y))], np.float32)
    return mat, (math.ceil(dst_width), math.ceil(dst_height))


def external_box(mask):
    """Mask.to_external_box: (up, down, left, right) of the pixels > 0"""
    rows, cols = np.nonzero((mask > 0).any(axis=1))[0], np.nonzero((mask > 0).any(axis=0))[0]
    if len(rows) == 0:
        raise RuntimeError('to_external_box: empty np_mask.')
    return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def warp_pair(image, mask, mat, dsize, extract=False):
    """rotate.distort of an image and its mask; extract: Mask.extract_image first"""
    if extract:
        image = image * (mask > 0)[:, :, None].astype(np.uint8)
    return O.warp_affine(np.ascontiguousarray(image), mat, dsize), O.warp_affine(np.ascontiguousarray(mask), mat, dsize)


def flatten(page, mask, box, angle):
    """one region of build_flattened_text_regions: box (up, down, left, right) of the box-attached mask"""
    up, down, left, right = box
    mat, dsize = rotate_matrix(angle, mask.shape)
    image, rotated = warp_pair(page[up:down + 1, left:right + 1], mask, mat, dsize, extract=True)
    t_up, t_down, t_left, t_right = external_box(rotated)
    # Image.to_cropped_image: `down or height - 1`, `right or width - 1`
    image = image[t_up:(t_down or image.shape[0] - 1) + 1, t_left:(t_right or image.shape[1] - 1) + 1]
    return dict(shape_before_trim=(dsize[1], dsize[0]), rotated_trimmed_box=(t_up, t_down, t_left, t_right), image=image,
                mask=rotated[t_up:t_down + 1, t_left:t_right + 1])


def resized_shape(height, width, resized_height, resized_width):
    if resized_height is None:
        resized_height = round(resized_width * height / width)
    if resized_width is None:
        resized_width = round(resized_height * width / height)
    return resized_height, resized_width


def resize_pair(image, mask, resized_height, resized_width):
    image_shape = resized_shape(image.shape[0], image.shape[1], resized_height, resized_width)
    mask_shape = resized_shape(mask.shape[0], mask.shape[1], resized_height, resized_width)
    plane = O.resize_cubic(np.ascontiguousarray((mask > 0).astype(np.uint8) * 255), mask_shape)
    return O.resize_cubic(np.ascontiguousarray(image), image_shape), (plane > 0).astype(np.uint8)


def post_rotate_pair(image, mask, angle):
    mat, dsize = rotate_matrix(angle, mask.shape)
    return warp_pair(image, mask, mat, dsize)


def background(height, width):
    rows = [np.zeros((width, 3), np.uint8) for _ in range(3)]
    colours = [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    for offset, row in enumerate(rows):
        for k in range(3):
            row[k::3] = colours[(offset + k) % 3]
    image = np.zeros((height, width, 3), np.uint8)
    for offset, row in enumerate(rows):
        image[offset::3] = row
    return image


def stack(shape, regions, origins):
    """the fills of stack_flattened_text_regions: regions [(image, mask)], origins [(up, left)], in order"""
    image, active = background(*shape), np.zeros(shape, np.uint8)
    for (region, mask), (up, left) in zip(regions, origins):
        h, w = mask.shape
        keep = mask > 0
        image[up:up + h, left:left + w][keep] = region[keep]
        active[up:up + h, left:left + w][keep] = 1
    return image, active


def load_golden():
    """tests/golden/text_region_flatten.npz -> (runs with their arrays in place, the 7 x 11 background)"""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'text_region_flatten.npz'))
    flats = {k: z[k] for k in z.files if k not in ('index', 'background_7x11')}

    def resolve(v):
        if isinstance(v, list) and len(v) == 3 and isinstance(v[1], list) and isinstance(v[2], str) and v[2] in flats:
            at, shape, dtype = v
            return flats[dtype][at:at + int(np.prod(shape))].reshape(shape)
        if isinstance(v, dict):
            return {k: resolve(x) for k, x in v.items()}
        if isinstance(v, list):
            return [resolve(x) for x in v]
        return v

    return [resolve(row) for row in json.loads(str(z['index']))['runs']], z['background_7x11']


class ReplayPacker:
    """a packer that answers with stored placements (bin, x, y, width, height, rid)"""

    def __init__(self, placements):
        self.placements, self.rects = [tuple(p) for p in placements], []

    def add_rect(self, width, height, rid=None):
        self.rects.append((width, height, rid))

    def add_bin(self, width, height):
        pass

    def pack(self):
        assert sorted(self.rects, key=lambda r: r[2]) == sorted(((p[3], p[4], p[5]) for p in self.placements), key=lambda r: r[2])

    def rect_list(self):
        return list(self.placements)
