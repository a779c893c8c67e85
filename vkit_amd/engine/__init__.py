"""Label engines (reference: vkit/engine/).  Only the char-mask engines are here, with the slice of the reference's engine
framework they need (engine/interface.py: ``create_engine_executor({'type': ..., 'config': {...}})`` and ``run``)."""
