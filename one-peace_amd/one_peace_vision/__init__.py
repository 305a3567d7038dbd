"""The vision branch on its own: the ImageNet classifier OnePeaceViT (one_peace_vision/classification of the reference), the checkpoint
surgery that cuts a pretraining checkpoint down to it and the layer-wise parameter groups it is fine-tuned with; and the video backbone
OnePeaceVideoViT (one_peace_vision/video) with its adapters, temporal attention, checkpoint loading and freezing rule; and the detection
backbone OnePeaceDetViT (one_peace_vision/det) with window attention, the decomposed relative positions and its checkpoint loading."""
from .det_vit import OnePeaceDetViT, get_onepeace_lr_decay_rate, load_pretrained_det  # noqa: F401
from .models_vit import (OnePeaceViT, convert_to_vision, get_layer_id_for_vit, load_pretrained, one_piece_g_256,  # noqa: F401
                         one_piece_g_384, one_piece_g_448, one_piece_g_512, param_groups_lrd, vision_param_groups)
from .video_vit import (Adapter, OnePeaceVideoViT, VideoEncoderLayer, VideoImageAdapter, VideoRecognizer,  # noqa: F401
                        freeze_for_adapters)
from .video_vit import load_pretrained as load_pretrained_video  # noqa: F401
