"""Decoded textures of the image engines, kept on the device: least recently used first out, bounded by a byte budget."""
from collections import OrderedDict


class TextureCache:
    """key -> DevArray.  A texture dropped here stays alive for whoever still holds it (a run keeps the textures of its launch
    until the launch is queued; the block returns to the context's pool when the last holder lets go)."""

    def __init__(self, budget_bytes: int):
        self.budget_bytes = int(budget_bytes)
        self.items = OrderedDict()
        self.bytes = 0

    def get(self, key):
        arr = self.items.get(key)
        if arr is not None:
            self.items.move_to_end(key)
        return arr

    def put(self, key, arr):
        old = self.items.pop(key, None)
        if old is not None:
            self.bytes -= old.nbytes
        self.items[key] = arr
        self.bytes += arr.nbytes
        while self.bytes > self.budget_bytes and self.items:
            _, dropped = self.items.popitem(last=False)
            self.bytes -= dropped.nbytes
        return arr

    def __len__(self):
        return len(self.items)
