from .embedding_loss import EmbeddingLoss, EmbeddingLossFunction  # noqa: F401
from .cross_entropy import CrossEntropyLoss  # noqa: F401
