"""Mirror of one_peace/metrics/accuracy.py (``Accuracy``): top-1 accuracy of classification logits, as the reference's classification
and VQA tasks validate (1-D class targets, or 2-D soft-label targets whose entry at the predicted class is the score).  Same keys,
same values; the state lives on the device of the inputs instead of a hard-coded .cuda()."""
import torch
import torch.distributed as dist

from .recall import gather_variable


def _distributed():
    return dist.is_available() and dist.is_initialized()


class Accuracy:
    """initialize() once per validation; compute(ids, logits, targets) per batch; merge_results() sums the counts over the ranks,
    gathers ids and predictions in rank order and returns the eval_log (the same on every rank)."""

    def initialize(self):
        self.score_sum = torch.zeros(1, dtype=torch.float32)
        self.score_cnt = torch.zeros(1, dtype=torch.int32)
        self.ids = torch.zeros(0, dtype=torch.long)
        self.hyps = torch.zeros(0, dtype=torch.long)

    def _to(self, device):
        if self.score_sum.device != device:
            self.score_sum, self.score_cnt = self.score_sum.to(device), self.score_cnt.to(device)
            self.ids, self.hyps = self.ids.to(device), self.hyps.to(device)

    def compute(self, ids, logits, targets):
        self._to(logits.device)
        predict_labels = logits.argmax(1)
        if targets.dim() == 2:
            n_correct = targets.gather(1, predict_labels.unsqueeze(1)).sum()
        else:
            n_correct = predict_labels.eq(targets).sum()
        self.score_sum += n_correct
        self.score_cnt += logits.size(0)
        self.ids = torch.cat([self.ids, ids], dim=0)
        self.hyps = torch.cat([self.hyps, predict_labels], dim=0)

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
        return {"accuracy": score_sum / score_cnt, "score_sum": score_sum, "score_cnt": score_cnt, "predict_results": predict_results}
