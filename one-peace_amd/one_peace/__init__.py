from . import one_peace_base, one_peace_retrieval, one_peace_pretrain, one_peace_classify, hub_interface  # noqa: F401  (fills the registries)
