"""The vision branch on its own (one_peace_vision/classification of the reference): the ImageNet classifier OnePeaceViT, the checkpoint
surgery that cuts a pretraining checkpoint down to it, and the layer-wise parameter groups it is fine-tuned with."""
from .models_vit import (OnePeaceViT, convert_to_vision, get_layer_id_for_vit, load_pretrained, one_piece_g_256,  # noqa: F401
                         one_piece_g_384, one_piece_g_448, one_piece_g_512, param_groups_lrd, vision_param_groups)
