from .embedding_loss import EmbeddingLoss, EmbeddingLossFunction  # noqa: F401
