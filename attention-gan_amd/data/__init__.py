__all__ = ["batches", "captions"]
from . import batches, captions  # noqa: F401,E402
