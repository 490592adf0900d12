"""Key strings of the model's output dict (utils/constants.py:15-46), with the reference's values."""


class Loss(object):
    EMBEDDING = "embedding_loss"
    SEMSEG = "semantic_segmentation_loss"
    FOREGROUND = "foreground"
    LOVASZ_LOSS = "lovasz_loss"
    SEEDINESS_LOSS = "seediness_loss"
    VARIANCE_SMOOTHNESS = "variance_smoothness_loss"

    def __init__(self):
        raise ValueError("Static class 'Losses' should not be instantiated")


class ModelOutput(object):
    SEMSEG_MASKS = "semseg_masks",          # (a one-tuple in the reference too: constants.py:32-33, trailing commas)
    EMBEDDINGS = "embeddings",
    INFERENCE = "inference"
    OPTIMIZATION_LOSSES = "optimization_losses"
    OTHERS = "others"

    def __init__(self):
        raise ValueError("Static class 'ModelOutput' should not be instantiated")
