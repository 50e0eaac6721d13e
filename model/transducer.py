from conformer_amd.model.transducer import ConformerTransducer  # noqa: F401
