"""Mirror of one_peace/metrics: the retrieval metric, scored through ops.similarity_topk."""
from .recall import Recall, gather_variable  # noqa: F401
