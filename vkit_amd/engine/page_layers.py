"""The small layers of a page -- non-text symbols, barcode score maps, text-line bounding-box frames -- planned on the host and
rendered by ONE ``vkx_page_layers_dev`` call (csrc/page_layers.hip): at most two launches whatever the number of layers, no
synchronisation.  The barcode engines (``vkit_amd.engine.barcode``) and the steps PageBarcodeStep, PageTextLineBoundingBoxStep
and PageNonTextSymbolStep add their plans to a ``LayerBatch`` and take the planes it renders: views of one packed device block in
``_native.resident(True)``, slices of its one download otherwise."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from vkit_amd import _native


def _align(n: int) -> int:
    return (n + 255) & ~255


class LayerBatch:

    def __init__(self):
        self.records: List[dict] = []
        self.sources: List[np.ndarray] = []     # host sources, in blob order
        self.blob_bytes = 0
        self.dst_bytes = 0
        self.keep = []                          # device sources stay alive until the call is queued

    def __len__(self):
        return len(self.records)

    def _take(self, nbytes: int) -> int:
        off = self.dst_bytes
        self.dst_bytes = _align(off + nbytes)
        return off

    def _source(self, record: dict, src, shape: Tuple[int, ...]):
        if isinstance(src, _native.DevArray):
            if tuple(src.shape) != shape or src.dtype != np.uint8:
                raise ValueError(f'source {tuple(src.shape)} {src.dtype} is not uint8 {shape}')
            self.keep.append(src)
            record.update(src_off=-1, src_dev=src.ptr)
            return
        src = np.ascontiguousarray(src)
        if src.shape != shape or src.dtype != np.uint8:
            raise ValueError(f'source {src.shape} {src.dtype} is not uint8 {shape}')
        record.update(src_off=self.blob_bytes, src_dev=0)
        self.sources.append(src)
        self.blob_bytes = _align(self.blob_bytes + src.nbytes)

    def _add(self, kind: int, src_shape, out_shape, alpha: float, with_image: bool, **fields) -> int:
        out_h, out_w = int(out_shape[0]), int(out_shape[1])
        record = dict(kind=kind, src_h=int(src_shape[0]), src_w=int(src_shape[1]), out_h=out_h, out_w=out_w, alpha=float(alpha),
                      src_off=-1, src_dev=0, image_off=0, **fields)
        if with_image:
            record['image_off'] = self._take(3 * out_h * out_w)
        record['alpha_off'] = self._take(4 * out_h * out_w)
        self.records.append(record)
        return len(self.records) - 1

    def add_symbol_rgba(self, src, out_shape, alpha: float) -> int:
        """``src`` uint8 (sh, sw, 4), host or DevArray -> image (oh, ow, 3) and alpha plane (oh, ow)."""
        index = self._add(_native.LAYER_SYMBOL_RGBA, src.shape, out_shape, alpha, True)
        self._source(self.records[index], src, (src.shape[0], src.shape[1], 4))
        return index

    def add_symbol_gray(self, src, out_shape, alpha: float, color: Sequence[int]) -> int:
        """``src`` uint8 (sh, sw) -> the constant ``color`` image and the plane alpha where the resized symbol is > 0."""
        index = self._add(_native.LAYER_SYMBOL_GRAY, src.shape, out_shape, alpha, True, color=tuple(int(c) for c in color))
        self._source(self.records[index], src, (src.shape[0], src.shape[1]))
        return index

    def add_score(self, mask: np.ndarray, out_shape, alpha: float) -> int:
        """``mask`` uint8 0 / 1 module mask (sh, sw) -> the score map (oh, ow): alpha on the modules, resized and clipped."""
        index = self._add(_native.LAYER_SCORE, mask.shape, out_shape, alpha, False)
        self._source(self.records[index], mask, (mask.shape[0], mask.shape[1]))
        return index

    def add_frame(self, box_shape, thickness: int, alpha: float, trims: Sequence[int]) -> int:
        """A ring of ``thickness`` around 0 on a plane of ``box_shape``, trimmed by ``trims`` (up, down, left, right)."""
        up, down, left, right = (int(t) for t in trims)
        out_shape = (int(box_shape[0]) - up - down, int(box_shape[1]) - left - right)
        return self._add(_native.LAYER_FRAME, box_shape, out_shape, alpha, False, thickness=int(thickness), trim=(up, down, left, right))

    def tables(self):
        """``(records, blob)``: the PAGE_LAYER_DTYPE table and the uint8 host block of ``vkx_page_layers_dev``."""
        table = np.zeros(len(self.records), _native.PAGE_LAYER_DTYPE)
        for row, record in zip(table, self.records):
            for name, value in record.items():
                row[name] = value
        blob = np.zeros(self.blob_bytes, np.uint8)
        for record, src in zip((r for r in self.records if r['src_off'] >= 0), self.sources):
            blob[record['src_off']:record['src_off'] + src.nbytes] = src.reshape(-1)
        return table, blob

    def render(self, ctx=None, resident: Optional[bool] = None):
        """Every layer in one call -> per layer ``(image or None, plane)``: DevViews of the packed block when ``resident`` (default:
        ``_native.resident_mode()``), else host arrays cut from its one download."""
        if not self.records:
            return []
        if resident is None:
            resident = _native.resident_mode()
        ctx = ctx or (self.keep[0].ctx if self.keep else _native.default_ctx())
        table, blob = self.tables()
        dst = ctx.dev_empty((self.dst_bytes,), np.uint8)
        _native.page_layers(table, blob, dst)
        self.keep = []
        host = None if resident else dst.host()
        out = []
        for record in self.records:
            shape = (record['out_h'], record['out_w'])
            image = None
            if record['kind'] in (_native.LAYER_SYMBOL_RGBA, _native.LAYER_SYMBOL_GRAY):
                image = self._plane(dst, host, record['image_off'], shape + (3,), np.uint8)
            out.append((image, self._plane(dst, host, record['alpha_off'], shape, np.float32)))
        return out

    @staticmethod
    def _plane(dst, host, off, shape, dtype):
        if host is None:
            return _native.DevView(dst, off, shape, dtype)
        count = int(np.prod(shape))
        # (a copy: the page-locked download belongs to the block, the planes to their elements)
        return np.array(host[off:off + count * np.dtype(dtype).itemsize].view(dtype).reshape(shape))
