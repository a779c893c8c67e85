"""The font engine without its rasteriser (reference: vkit/engine/font/): the containers of ``type.py`` and the text-line half of
``freetype.py`` -- glyph bitmaps to a ``TextLine``, planned on the host and rendered on the GPU (``text_line.py``).  Glyph
rasterisation (freetype) stays outside: ``render_text_line_meta`` takes it as a callable."""
from .type import (
    CharBox,
    CharGlyph,
    FontEngineRunConfig,
    FontEngineRunConfigGlyphSequence,
    FontEngineRunConfigStyle,
    FontGlyphInfo,
    FontGlyphInfoCollection,
    FontVariant,
    TextLine,
)
from .text_line import (
    TextLineBatch,
    TextLineHandle,
    TextLinePlan,
    build_char_glyph,
    build_text_line_tables,
    estimate_font_size,
    get_kerning_limits_hori_default,
    lcd_paste_plane,
    place_char_glyphs_in_text_line_hori_default,
    place_char_glyphs_in_text_line_vert_default,
    plan_text_line,
    render_char_glyphs_from_text,
    render_text_line_meta,
    render_text_line_plans,
    resize_and_trim_text_line_hori_default,
    resize_and_trim_text_line_vert_default,
    trim_char_np_image_hori,
    trim_char_np_image_vert,
)

__all__ = ['CharBox', 'CharGlyph', 'FontEngineRunConfig', 'FontEngineRunConfigGlyphSequence', 'FontEngineRunConfigStyle', 'FontGlyphInfo',
           'FontGlyphInfoCollection', 'FontVariant', 'TextLine', 'TextLineBatch', 'TextLineHandle', 'TextLinePlan', 'build_char_glyph',
           'build_text_line_tables', 'estimate_font_size', 'get_kerning_limits_hori_default', 'lcd_paste_plane',
           'place_char_glyphs_in_text_line_hori_default', 'place_char_glyphs_in_text_line_vert_default', 'plan_text_line',
           'render_char_glyphs_from_text', 'render_text_line_meta', 'render_text_line_plans', 'resize_and_trim_text_line_hori_default',
           'resize_and_trim_text_line_vert_default', 'trim_char_np_image_hori', 'trim_char_np_image_vert']
