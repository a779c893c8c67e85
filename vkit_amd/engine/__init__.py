"""Engines (reference: vkit/engine/).  The char-mask engines (``char_mask``: ``default``, ``external_ellipse``), the default
char-heatmap engine (``char_heatmap``), the image engines (``image``: ``combiner``, ``selector``), the seal-impression engine
(``seal_impression``: ``ellipse``, and ``fill_text_line_to_seal_impression``), the barcode engines (``barcode``: ``qr``, ``code39``,
their encoders injected; ``page_layers``: the batch their score maps, the frames and the symbols of a page are rendered by) and the containers of a font engine's output
(``font``) are here, with the slice of
the reference's engine framework they need (engine/interface.py: ``create_engine_executor({'type': ..., 'config': {...}})`` for
the char masks, ``char_heatmap_default_engine_executor_factory.create(init_config)`` for the heatmap, and in ``interface`` the
general ``type / weight / config`` aggregator the image engines are drawn from)."""
