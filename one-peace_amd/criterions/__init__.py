from . import contrastive, finetune, pretrain  # noqa: F401  (fills the criterion registries)
