from conformer_amd.model.wav2vec2 import Wav2Vec2  # noqa: F401
