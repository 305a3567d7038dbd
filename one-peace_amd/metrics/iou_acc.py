"""Mirror of one_peace/metrics/iou_acc.py (``IouAcc``): the share of predicted boxes (x0, y0, x1, y1) whose IoU with the target box is
at least 0.5 AND whose intersection has positive width and height, as the reference's grounding task validates.  Same keys, same
values; the state lives on the device of the inputs instead of a hard-coded .cuda()."""
import torch
import torch.distributed as dist

from .accuracy import _distributed
from .recall import gather_variable


class IouAcc:
    """initialize() once per validation; compute(ids, hyps, refs) per batch of boxes [B, 4]; merge_results() sums the counts over the
    ranks, gathers ids and boxes in rank order and returns the eval_log (the same on every rank)."""

    def initialize(self):
        self.ids = torch.zeros(0, dtype=torch.float32)   # the reference's torch.Tensor([]): ids come out as floats
        self.hyps = torch.zeros(0, dtype=torch.float32)
        self.score_sum = torch.zeros(1, dtype=torch.float32)
        self.score_cnt = torch.zeros(1, dtype=torch.int32)

    def _to(self, device):
        if self.score_sum.device != device:
            self.score_sum, self.score_cnt = self.score_sum.to(device), self.score_cnt.to(device)
            self.ids, self.hyps = self.ids.to(device), self.hyps.to(device)

    def compute(self, ids, hyps, refs):
        self._to(hyps.device)
        interacts = torch.cat([torch.where(hyps[:, :2] < refs[:, :2], refs[:, :2], hyps[:, :2]),
                               torch.where(hyps[:, 2:] < refs[:, 2:], hyps[:, 2:], refs[:, 2:])], dim=1)
        area_predictions = (hyps[:, 2] - hyps[:, 0]) * (hyps[:, 3] - hyps[:, 1])
        area_targets = (refs[:, 2] - refs[:, 0]) * (refs[:, 3] - refs[:, 1])
        interacts_w = interacts[:, 2] - interacts[:, 0]
        interacts_h = interacts[:, 3] - interacts[:, 1]
        area_interacts = interacts_w * interacts_h
        ious = area_interacts.float() / (area_predictions + area_targets - area_interacts)
        self.score_sum += ((ious >= 0.5) & (interacts_w > 0) & (interacts_h > 0)).float().sum()
        self.score_cnt += hyps.size(0)
        self.ids = torch.cat([self.ids, ids], dim=0)
        self.hyps = torch.cat([self.hyps, hyps], dim=0)  # (torch.cat skips the empty 1-D start, as in the reference)

    def merge_results(self, output_predict=False):
        score_sum, score_cnt = self.score_sum.clone(), self.score_cnt.clone()
        if _distributed():
            dist.all_reduce(score_sum, op=dist.ReduceOp.SUM)
            dist.all_reduce(score_cnt, op=dist.ReduceOp.SUM)
        ids, hyps = gather_variable(self.ids), gather_variable(self.hyps)
        predict_results = {}
        if output_predict:
            for id, hyp in zip(ids.cpu().tolist(), hyps.cpu().tolist()):
                predict_results[id] = hyp
        score_sum, score_cnt = score_sum.item(), score_cnt.item()
        return {"iou_acc": score_sum / score_cnt, "score_sum": score_sum, "score_cnt": score_cnt, "predict_results": predict_results}
