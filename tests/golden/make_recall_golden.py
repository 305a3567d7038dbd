"""Generate tests/golden/recall.pt from the UNMODIFIED reference metric (one_peace/metrics/recall.py, class Recall), run on CPU
through oracle/ref_shim.py.

    python tests/golden/make_recall_golden.py        # needs the reference tree; writes tests/golden/recall.pt

recall.py imports all_gather from ..utils.data_utils, which it only calls under torch.distributed; that one name is stubbed here.
Data: 16 images (3 without a caption), 5 captions per captioned image, 64-dim embeddings of small integers times 1/8 -- exact in
bf16, every dot product exact in fp32 -- chosen so that in every row of both score matrices the 11 best scores are distinct (gaps
>= 1/64), so no accumulation order can reorder them.  The file holds tensors and plain numbers only.
"""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402

N_IMG, N_CAPTIONED, PER, D = 16, 13, 5, 64


def reference_recall():
    R.install()
    op_root = os.path.join(R.REFERENCE_ROOT, "one_peace")
    for name, path in (("one_peace.metrics", os.path.join(op_root, "metrics")), ("one_peace.utils", os.path.join(op_root, "utils"))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [path]
            m.__package__ = name
            sys.modules[name] = m
    stub = types.ModuleType("one_peace.utils.data_utils")

    def all_gather(q, exclude_self=False):
        raise RuntimeError("not reached: the fixture runs without torch.distributed")

    stub.all_gather = all_gather
    sys.modules["one_peace.utils.data_utils"] = stub
    return importlib.import_module("one_peace.metrics.recall").Recall


def separated(scores, top=11):
    v = torch.sort(scores, dim=1, descending=True)[0][:, :top]
    return bool((v[:, :-1] - v[:, 1:] > 1e-3).all())


def make_data():
    for seed in range(1000):
        g = torch.Generator().manual_seed(seed)
        img = torch.randint(-30, 31, (N_IMG, D), generator=g).float()
        txt = img[:N_CAPTIONED].repeat_interleave(PER, 0) + torch.randint(-100, 101, (N_CAPTIONED * PER, D), generator=g).float()
        img, txt = img / 8, txt / 8
        s = img.double() @ txt.double().t()
        if separated(s) and separated(s.t()):
            assert torch.equal(img.to(torch.bfloat16).float(), img) and torch.equal(txt.to(torch.bfloat16).float(), txt)
            image_ids = 1000 + 3 * torch.arange(N_IMG)
            text_ids = image_ids[:N_CAPTIONED].repeat_interleave(PER)
            return image_ids, img, text_ids, txt, seed
    raise RuntimeError("no separated draw")


def main():
    Recall = reference_recall()
    image_ids, img, text_ids, txt, seed = make_data()
    r = Recall()
    r.initialize(text_ids, txt)
    r.compute(image_ids[:7], img[:7])
    r.compute(image_ids[7:], img[7:])
    log = r.merge_results(output_predict=True)
    out = {"seed": seed, "image_ids": image_ids, "image_emb": img, "text_ids": text_ids, "text_emb": txt, "eval_log": log}
    torch.save(out, os.path.join(HERE, "recall.pt"))
    print({k: v for k, v in log.items() if not k.startswith("predict")})


if __name__ == "__main__":
    main()
