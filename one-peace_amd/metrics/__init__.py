"""Mirror of one_peace/metrics: the retrieval metric, scored through ops.similarity_topk, and the classification metrics -- top-1
accuracy, IoU accuracy of boxes, and mean average precision through ops.average_precision."""
from .recall import Recall, gather_variable  # noqa: F401
from .accuracy import Accuracy  # noqa: F401
from .iou_acc import IouAcc  # noqa: F401
from .map import MAP  # noqa: F401
