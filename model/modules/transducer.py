from conformer_amd.model.modules.transducer import Joiner, Predictor  # noqa: F401
