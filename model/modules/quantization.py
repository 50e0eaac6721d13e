from conformer_amd.model.modules.quantization import Quantization  # noqa: F401
