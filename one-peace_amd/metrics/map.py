"""Mirror of one_peace/metrics/map.py (``MAP``): mean average precision over the classes of a multi-label task, as the reference
validates audio tagging (tasks/audio_tasks/fsd50k.py).

The reference copies sigmoid(logits) to the host and calls sklearn's average_precision_score per class (map.py:35-44).  Here the
sigmoid runs in fp32 on the logits' device exactly as there -- distinct confident logits collapse to equal fp32 sigmoid values, and
that tie structure is part of the reference's result -- and the per-class average precision comes from ops.average_precision
(op_average_precision on a CUDA device: no host copy, no sort, no sklearn).  Same keys; `map` is the fp64 mean over the classes."""
import torch

from .. import ops
from .recall import gather_variable


class MAP:
    """initialize() once per validation; compute(ids, logits, targets) per batch (logits and 0 / 1 targets [B, C]); merge_results()
    gathers all three across the ranks in rank order and returns the eval_log (the same on every rank)."""

    def initialize(self):
        self.logits = torch.zeros(0, dtype=torch.float32)
        self.targets = torch.zeros(0, dtype=torch.float32)
        self.ids = torch.zeros(0, dtype=torch.long)

    def compute(self, ids, logits, targets):
        if self.logits.device != logits.device:
            self.logits, self.targets, self.ids = (t.to(logits.device) for t in (self.logits, self.targets, self.ids))
        self.ids = torch.cat([self.ids, ids], dim=0)
        self.logits = torch.cat([self.logits, logits], dim=0)
        self.targets = torch.cat([self.targets, targets], dim=0)

    def merge_results(self, output_predict=False):
        ids = gather_variable(self.ids)
        preds = torch.sigmoid(gather_variable(self.logits))
        targets = gather_variable(self.targets)
        ap, _ = ops.average_precision(preds, targets)
        predict_results = {}
        if output_predict:
            for id, pred in zip(ids.cpu().tolist(), preds.cpu().tolist()):
                predict_results[id] = pred
        return {"map": ap.mean().item(), "map_cnt": len(targets), "predict_results": predict_results}
