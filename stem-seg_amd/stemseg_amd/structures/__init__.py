from .image_list import ImageList  # noqa: F401
