"""Fine-tuning criteria, mirroring one_peace/criterions/{classify_loss,hinge_loss,refcoco_loss}.py: `classify_criterion` (vqa, nlvr2,
vggsound, fsd50k, image classification), `hinge_loss` (aqa) and `refcoco_criterion` (visual grounding).

``forward(model, sample, reduce=True) -> (loss, sample_size, logging_output)`` with the reference's keys and sample sizes.  The criteria
only call ``model(**net_input)`` and take logits, so any module that returns [B, C] logits will do.  What is MI355X design and not
semantics: on bf16 / fp32 device logits the loss, the logged counter and the gradient come from one pass of the HIP loss kernels
(ops.classify_loss, ops.hinge_loss, ops.box_loss), the loss and `n_correct` are fp32 whatever the logits' dtype, and two runs give
the same bits.  One deviation: `HingeLoss` honours its `margin` option, which the reference accepts and then ignores (it hard-codes
``1 +``); the two agree at the default 1.0."""
from .. import ops
from ..registry import FairseqCriterion, register_criterion

try:
    from fairseq import metrics as _metrics  # type: ignore
except Exception:
    _metrics = None


def _item(x):
    return x.item() if hasattr(x, "item") else x


def _reduce_loss(logging_outputs):
    """The part the three reduce_metrics share; returns sample_size."""
    tot = lambda k: sum(log.get(k, 0) for log in logging_outputs)  # noqa: E731
    loss_sum, nsentences, sample_size = tot("loss"), tot("nsentences"), tot("sample_size")
    _metrics.log_scalar("loss", loss_sum / sample_size, sample_size, round=3)
    _metrics.log_scalar("nsentences", nsentences, 1, round=3)
    _metrics.log_scalar("sample_size", sample_size, 1, round=3)
    return sample_size


class _CountingCriterion(FairseqCriterion):
    """loss + n_correct criteria: sample_size = nsentences, accuracy = n_correct / total."""

    @staticmethod
    def _outputs(loss, n_correct, sample):
        sample_size = sample["nsentences"]
        logging_output = {"loss": loss.data, "nsentences": sample["nsentences"], "sample_size": sample_size, "n_correct": n_correct}
        return loss, sample_size, logging_output

    @staticmethod
    def reduce_metrics(logging_outputs) -> None:
        if _metrics is None:
            return
        total = _item(_reduce_loss(logging_outputs))
        if total > 0:
            _metrics.log_scalar("total", total)
            _metrics.log_scalar("n_correct", _item(sum(log.get("n_correct", 0) for log in logging_outputs)))
            _metrics.log_derived(
                "accuracy",
                lambda meters: round(meters["n_correct"].sum * 100.0 / meters["total"].sum, 3) if meters["total"].sum > 0 else float("nan"))

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True


@register_criterion("classify_criterion")
class ClassifyCriterion(_CountingCriterion):
    def __init__(self, task, use_multi_label=False, label_smoothing=0.0):
        super().__init__(task)
        self.use_multi_label = use_multi_label
        self.label_smoothing = label_smoothing

    def forward(self, model, sample, reduce=True):
        logits = model(**sample["net_input"])
        loss, n_correct = ops.classify_loss(logits, sample["target"], self.use_multi_label, self.label_smoothing)
        return self._outputs(loss, n_correct, sample)


@register_criterion("hinge_loss")
class HingeLoss(_CountingCriterion):
    def __init__(self, task, margin=1.0, num_choices=4):
        super().__init__(task)
        self.margin = margin
        self.num_choices = num_choices

    def forward(self, model, sample, reduce=True):
        ni = sample["net_input"]
        src_audios = ni["src_audios"].repeat_interleave(self.num_choices, 0)
        audio_padding_masks = ni["audio_padding_masks"].repeat_interleave(self.num_choices, 0)
        logits = model(src_tokens=ni["src_tokens"], src_audios=src_audios, audio_padding_masks=audio_padding_masks).view(-1, self.num_choices)
        loss, n_correct = ops.hinge_loss(logits, sample["target"], self.margin)
        return self._outputs(loss, n_correct, sample)


@register_criterion("refcoco_criterion")
class RefCOCOCriterion(FairseqCriterion):
    def __init__(self, task):
        super().__init__(task)

    def forward(self, model, sample, reduce=True):
        logits = model(**sample["net_input"])
        if sample["nsentences"] == logits.shape[0]:
            loss = ops.box_loss(logits, sample["target"])
        else:  # the L1 term is divided by nsentences, whatever the batch holds
            loss = ops.box_loss_torch(logits, sample["target"], sample["nsentences"])
        sample_size = 1
        logging_output = {"loss": loss.data, "nsentences": sample["nsentences"], "sample_size": sample_size}
        return loss, sample_size, logging_output

    @staticmethod
    def reduce_metrics(logging_outputs) -> None:
        if _metrics is None:
            return
        _reduce_loss(logging_outputs)

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True
