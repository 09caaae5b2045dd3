"""`mindspore.nn.layer`."""
from . import basic, embedding  # noqa: F401
from .basic import ClipByNorm, Dense, Dropout, Flatten, MatMul  # noqa: F401
from .embedding import EmbeddingLookup  # noqa: F401
