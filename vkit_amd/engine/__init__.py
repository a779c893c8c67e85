"""Label engines (reference: vkit/engine/).  The char-mask engines (``char_mask``: ``default``, ``external_ellipse``) and the
default char-heatmap engine (``char_heatmap``) are here, with the slice of the reference's engine framework they need
(engine/interface.py: ``create_engine_executor({'type': ..., 'config': {...}})`` for the char masks,
``char_heatmap_default_engine_executor_factory.create(init_config)`` for the heatmap, and ``run``)."""
