"""Mirror of one_peace/metrics/recall.py (``Recall``): recall@1/5/10 of image (or audio) -> text and text -> image retrieval, as the
reference's validation of the pretraining objective and its retrieval tasks compute it (image_text_pretrain.py:86-136,
audio_text_pretrain.py, image_text_retrieval.py, audio_text_retrieval.py).

The reference forms ``image_logits @ text_logits.t()`` and calls ``topk(10)`` on it in both directions (recall.py:31-51).  Here both
directions come from ``ops.similarity_topk`` -- op_sim_topk on bf16 CUDA embeddings, which never forms the score matrix -- and an id
gather.  Same keys, same values; exact ties rank the lower index first (torch.topk leaves their order unspecified)."""
import torch
import torch.distributed as dist

from .. import ops

RECALL_AT = (1, 5, 10)


def gather_variable(t):
    """All-gather of a tensor whose first dimension differs between ranks, in rank order (utils/data_utils.py:50-85, all_gather):
    the sizes first, every shard zero-padded to the largest, gathered, trimmed.  Returns ``t`` when no process group is up."""
    if not (dist.is_available() and dist.is_initialized()):
        return t
    world = dist.get_world_size()
    local = torch.tensor([t.shape[0]], dtype=torch.long, device=t.device)
    sizes = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(sizes, local)
    sizes = [int(s.item()) for s in sizes]
    top = max(sizes)
    if t.shape[0] < top:
        t = torch.cat([t, t.new_zeros((top - t.shape[0],) + tuple(t.shape[1:]))])
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return torch.cat([p[:n] for p, n in zip(parts, sizes)], dim=0)


class Recall:
    """initialize(text_ids, text_logits) once per validation (the text side, already gathered by the caller with gather_variable, as
    the reference tasks do in begin_valid_epoch); compute(ids, logits) per batch of images / audio clips; merge_results() gathers
    the query side across ranks and returns the eval_log (the same on every rank).  modality="audio" names the img_* keys audio_*,
    as audio_text_retrieval.py / audio_text_pretrain.py do in their merge_results."""

    def __init__(self, modality="image"):
        assert modality in ("image", "audio"), modality
        self.modality = modality

    def initialize(self, text_ids, text_logits):
        self.text_ids = text_ids
        self.text_logits = text_logits
        self.image_ids_list = []
        self.image_logits_list = []

    def compute(self, image_ids, image_logits):
        self.image_ids_list.append(image_ids)
        self.image_logits_list.append(image_logits)

    def merge_results(self, output_predict=False):
        image_ids = torch.cat(self.image_ids_list, dim=0)
        image_logits = torch.cat(self.image_logits_list, dim=0)
        self.image_ids = gather_variable(image_ids)
        self.image_logits = gather_variable(image_logits)
        stats = self.retrieval_eval(output_predict=output_predict)
        if self.modality == "audio":
            for key in list(stats.keys()):
                if key.startswith("img"):
                    stats[key.replace("img", "audio")] = stats.pop(key)
        return stats

    def retrieval_eval(self, scores_i2t=None, scores_t2i=None, output_predict=False):
        """recall.py:36-88 over the stored logits.  Score matrices, when a caller passes them as the reference does, are ranked with
        the same order (stable descending sort) instead."""
        n_img, n_txt = self.image_ids.shape[0], self.text_ids.shape[0]
        if scores_i2t is None:
            _, rank_txt = ops.similarity_topk(self.image_logits, self.text_logits, min(10, n_txt))
            _, rank_img = ops.similarity_topk(self.text_logits, self.image_logits, min(10, n_img))
        else:
            rank_txt = torch.sort(scores_i2t.float(), dim=1, descending=True, stable=True)[1][:, :10]
            rank_img = torch.sort(scores_t2i.float(), dim=1, descending=True, stable=True)[1][:, :10]
        text_ids = self.text_ids.to(rank_txt.device)
        image_ids = self.image_ids.to(rank_txt.device)
        predict_txt = text_ids[rank_txt]
        predict_img = image_ids[rank_img]
        i2t = [predict_txt[:, :r].eq(image_ids[:, None]).any(1).sum().item() for r in RECALL_AT]
        t2i = [predict_img[:, :r].eq(text_ids[:, None]).any(1).sum().item() for r in RECALL_AT]

        tr_r1, tr_r5, tr_r10 = (100.0 * c / n_img for c in i2t)
        tr_mean = (tr_r1 + tr_r5 + tr_r10) / 3
        ir_r1, ir_r5, ir_r10 = (100.0 * c / n_txt for c in t2i)
        ir_mean = (ir_r1 + ir_r5 + ir_r10) / 3

        predict_txt_results, predict_img_results = {}, {}
        if output_predict:
            for img_id, p in zip(image_ids.cpu().tolist(), predict_txt.cpu().tolist()):
                predict_txt_results[img_id] = p
            for txt_id, p in zip(text_ids.cpu().tolist(), predict_img.cpu().tolist()):
                predict_img_results[txt_id] = p

        return {"txt_r1": tr_r1, "txt_r5": tr_r5, "txt_r10": tr_r10, "txt_r_mean": tr_mean, "img_count": n_img,
                "img_r1": ir_r1, "img_r5": ir_r5, "img_r10": ir_r10, "img_r_mean": ir_mean, "r_mean": (tr_mean + ir_mean) / 2,
                "txt_count": n_txt, "predict_txt": predict_txt_results, "predict_img": predict_img_results}
