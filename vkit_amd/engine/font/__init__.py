"""Containers for what a font engine produced (reference: vkit/engine/font/type.py).  No freetype and no rendering here: the
classes carry rendered glyphs and text lines into the engines that place them (``vkit_amd.engine.seal_impression``)."""
from .type import CharBox, CharGlyph, TextLine

__all__ = ['CharBox', 'CharGlyph', 'TextLine']
