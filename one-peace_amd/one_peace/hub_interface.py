"""Mirror of the feature-extraction surface of one_peace/models/one_peace/hub_interface.py:
``from_pretrained(...) -> OnePeaceHubInterface`` with ``extract_{text,image,audio,vl}_features`` (:206-225) and the dtype
cast of :107-122.  ``process_image`` (:150-168) takes image files, PIL images or decoded uint8 arrays and runs the reference's
transform (:94-101) -- on a device through the HIP resize kernel (ops.preprocess_images), bit for bit; ``process_text`` takes
token ids (no BPE) and does the collation only; ``process_audio`` (:170-193) takes WAV files, int16 PCM or float waveforms (no
librosa) and runs layer norm, crop, tiling and padding through ops.preprocess_audio, on a device in op_audio_normalize_pad; with
``resample=True`` clips at another rate are first resampled with this project's own low-pass (op_audio_resample), not soxr's."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from ..unify_model_config import one_peace_encoder_config
from .one_peace_classify import OnePeaceClassifyModel
from .one_peace_retrieval import OnePeaceRetrievalModel

_DTYPES = {"float32": torch.float32, "fp32": torch.float32, "fp16": torch.float16, "float16": torch.float16,
           "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


class _Dictionary:
    def __init__(self, n=50265, pad=1, bos=0, eos=2):
        self.n, self._pad, self._bos, self._eos = n, pad, bos, eos

    def __len__(self):
        return self.n

    def pad(self):
        return self._pad

    def bos(self):
        return self._bos

    def eos(self):
        return self._eos


def _cfg_get(tree, key, default=None):
    if isinstance(tree, dict):
        return tree.get(key, default)
    return getattr(tree, key, default)


_CLASSIFY_FIELDS = (("head_scale_ratio", 1), ("use_pooler", False), ("pooler_dropout", 0.0), ("attn_pooling", False),
                    ("use_image_features", False), ("freeze_finetune_updates", 0))


def build_from_checkpoint_cfg(model_cfg, head_type="vl", patch_image_size=256, vocab_size=50265, model_type="one_peace_retrieval",
                              num_classes=None, use_two_images=False):
    """Build the model from the `cfg.model` tree of a reference checkpoint (dict / namespace / omegaconf): the retrieval model, or
    with model_type="one_peace_classify" the fine-tuning model (num_classes / use_two_images are the task's, as in its build_model)."""
    enc = _cfg_get(model_cfg, "encoder")
    kw = {}
    for k in ("embed_dim", "ffn_embed_dim", "layers", "attention_heads", "drop_path_rate", "layer_scale_init_value"):
        v = _cfg_get(enc, k)
        if v is not None:
            kw[k] = v
    cfg_enc = one_peace_encoder_config(**kw)
    for k in ("magneto_scale_attn", "scale_attn", "scale_fc", "scale_heads", "use_layer_scale", "checkpoint_activations"):
        v = _cfg_get(enc, k)
        if v is not None:
            setattr(cfg_enc, k, v)
    for adapter in ("text_adapter", "image_adapter", "audio_adapter"):
        sub = _cfg_get(enc, adapter)
        if sub is not None:
            tgt = getattr(cfg_enc, adapter)
            for f in vars(tgt):
                v = _cfg_get(sub, f)
                if v is not None:
                    setattr(tgt, f, v)
    cfg_enc.image_adapter.rel_bucket_size = patch_image_size // 16
    if model_type == "one_peace_classify":
        cfg = SimpleNamespace(encoder=cfg_enc, **{k: type(d)(_cfg_get(model_cfg, k, d)) for k, d in _CLASSIFY_FIELDS})
        return OnePeaceClassifyModel(cfg, _Dictionary(vocab_size), head_type, num_classes=num_classes, use_two_images=use_two_images)
    if model_type != "one_peace_retrieval":
        raise NotImplementedError("from_pretrained: model_type %r (one_peace_retrieval or one_peace_classify)" % (model_type,))
    cfg = SimpleNamespace(encoder=cfg_enc, copy_rel_pos_table=bool(_cfg_get(model_cfg, "copy_rel_pos_table", False)))
    return OnePeaceRetrievalModel(cfg, _Dictionary(vocab_size), head_type)


def from_pretrained(model_name_or_path, model_type="one_peace_retrieval", device="cuda", dtype="float32",
                    download_root=None, head_type="vl", patch_image_size=256, num_classes=None, use_two_images=False):
    """hub_interface.py:53-73.  `model_name_or_path` must be a local checkpoint file ({"cfg": {"model": ...}, "model":
    state_dict}); downloading by name needs network access and the reference's URL table.  model_type="one_peace_classify" builds
    the fine-tuning model; head_type, num_classes and use_two_images are what the reference reads from the checkpoint's task."""
    ckpt = torch.load(model_name_or_path, map_location="cpu", weights_only=False)
    model_cfg = _cfg_get(_cfg_get(ckpt, "cfg"), "model")
    embed = ckpt["model"].get("encoder_wrapper.text_adapter.embed_tokens.weight")  # the dictionary's size, where there is a text tower
    model = build_from_checkpoint_cfg(model_cfg, head_type=head_type, patch_image_size=patch_image_size, model_type=model_type,
                                      num_classes=num_classes, use_two_images=use_two_images,
                                      vocab_size=embed.shape[0] if embed is not None else 50265)
    model.load_state_dict(ckpt["model"], strict=True)
    return OnePeaceHubInterface(model, device=device, dtype=dtype)


class OnePeaceHubInterface:
    def __init__(self, model, device="cuda", dtype="float32"):
        self.model = model.to(device).eval()
        self.device = device
        self.dtype = _DTYPES[dtype]
        self.dict = model.src_dict
        if self.dtype != torch.float32:  # hub_interface.py:107-114
            self.model.to(self.dtype)

    def cast_data_dtype(self, t):
        return t.to(self.dtype) if t.is_floating_point() else t

    # ---- collation of already pre-processed inputs -------------------------------------------------------------
    def process_text(self, token_id_lists):
        """list of 1-D LongTensors (BPE ids incl. EOS) -> right-padded [B, T] batch (collate_tokens semantics)."""
        T = max(len(t) for t in token_id_lists)
        out = torch.full((len(token_id_lists), T), self.dict.pad(), dtype=torch.long)
        for i, t in enumerate(token_id_lists):
            out[i, : len(t)] = t
        return out.to(self.device)

    @property
    def patch_image_size(self):
        """S of the image transform: the model's image adapter covers S / 16 patches per side (build_from_checkpoint_cfg)."""
        return int(self.model.cfg.encoder.image_adapter.rel_bucket_size) * 16

    def process_image(self, image_list, return_image_sizes=False):
        """hub_interface.py:150-168: Resize((S, S), BICUBIC) + ToTensor + Normalize(CLIP mean / std) of each image, stacked to
        [B, 3, S, S] on self.device in the hub dtype (S = patch_image_size); with return_image_sizes also the widths and heights of
        the inputs.  Items: file paths (decoded on the host with PIL, .convert("RGB")), PIL images, or uint8 [H, W, 3] RGB arrays /
        tensors (a uint8 [B, H, W, 3] batch works too; arrays never need PIL on a device).  On a device the resize and the
        normalisation run in op_image_resize_normalize (bit-identical to PIL + torchvision); on the CPU PIL does the resize.
        A floating-point tensor is taken as already pre-processed and only moved and cast, as before.
        The training transforms (RandomResizedCrop, Resize + CenterCrop, RandomHorizontalFlip) and Mixup / CutMix are
        augment.TrainImageTransform and augment.Mixup, on the same kernels; RandomDistortion / ColorJitter and GaussianBlur are
        augment.ColorJitter and augment.GaussianBlur (csrc/photometric.hip), the RefCOCO transform augment.GroundingTransform.
        Out of scope: JPEG / PNG decoding stays in PIL on the host; BPE for process_text, RandAugment, RandomErasing, timm's
        create_transform and hue jitter are not provided."""
        from .. import ops
        if torch.is_tensor(image_list) or isinstance(image_list, np.ndarray):
            batch = torch.as_tensor(image_list)
            if batch.is_floating_point():
                return self.cast_data_dtype(batch.to(self.device))
        items = [self._decoded(im) for im in image_list]
        widths = [im.size[0] if ops._is_pil(im) else int(im.shape[1]) for im in items]
        heights = [im.size[1] if ops._is_pil(im) else int(im.shape[0]) for im in items]
        src_images = ops.preprocess_images(items, self.patch_image_size, dtype=self.dtype, device=self.device)
        if return_image_sizes:
            return src_images, torch.tensor(widths).to(self.device), torch.tensor(heights).to(self.device)
        return src_images

    @staticmethod
    def _decoded(item):
        if isinstance(item, (str, bytes, os.PathLike)):
            from PIL import Image
            with Image.open(item) as im:
                return im.convert("RGB")
        return item

    def process_image_text_pairs(self, image_text_list, return_image_sizes=False):
        """hub_interface.py:195-204: ((src_images[, widths, heights]), src_tokens) of (image, token ids) pairs."""
        src_tokens = self.process_text([pair[1] for pair in image_text_list])
        images = [pair[0] for pair in image_text_list]
        if return_image_sizes:
            return self.process_image(images, return_image_sizes=True), src_tokens
        return self.process_image(images), src_tokens

    def _feature_encoder_spec(self):
        """The conv stack [(dim, kernel, stride), ...] of the model's audio adapter (hub_interface.py:116-118)."""
        cfg = getattr(getattr(self.model, "cfg", None), "encoder", None)
        spec = getattr(getattr(cfg, "audio_adapter", None), "feature_encoder_spec", None)
        return eval(spec) if isinstance(spec, str) else (spec or [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2)

    def _frames(self, n):
        """hub_interface.py:124-132 (_get_mask_indices_dims with padding 0, dilation 1)."""
        for _, k, s in self._feature_encoder_spec():
            n = 1 + (n - (k - 1) - 1) // s
        return n

    def process_audio(self, audio_list, sample_rate=16000, resample=False):
        """hub_interface.py:170-193: (src_audios [B, T], audio_padding_masks [B, frames + 1]) of audio clips.  Items, mixed freely:
        paths of 16-bit PCM WAV files (audioprep.read_wav), int16 PCM [n] / [n, 2], or float [n] / [n, C] arrays or tensors.  Per
        clip: mean over the channels, layer norm over the whole clip, crop to 15 s, tiling up to 1 s, an all-False frame mask of the
        clip's OWN length; then right-padding of the waveforms with 0 and of the masks with True (built on the host).
        An item may also be a (clip, rate) pair.  With resample=False a file or pair whose rate is not `sample_rate` raises
        ValueError("sample rate: R, need 16000"), as data/base_dataset.py:88-89.  With resample=True it is resampled first, as the
        reference's librosa.load(sr=16000) does (:175) -- but with the Kaiser-windowed sinc of audioprep.resample_filter
        (ops.resample_audio; on a device op_audio_resample, handed to the normalise kernel without leaving the device), not with
        librosa's soxr, which is not reproduced here: features of resampled audio differ from the reference's by the difference
        between the two low-pass filters.  The layer norm runs over the whole resampled clip before the crop (:176-182), and the
        frame masks come from the resampled lengths.  Clips at `sample_rate` are computed exactly as with resample=False.
        With device="cpu" this is ops.preprocess_audio's torch route, bit for bit what this method computed for 1-D float
        waveforms before it took files.  On a GPU device the same inputs go through op_audio_normalize_pad (csrc/audioprep.hip)
        and may differ from the host route by rounding: each fp32 value is within 2^-24 (4 |y| + 2 |mean| rstd) of the fp64
        result (torch's own fp32 layer norm was measured at up to 1.84 times that bound on the fixture's clips), before the cast to the
        hub dtype."""
        from .. import ops
        kdt = self.dtype if self.dtype in (torch.bfloat16, torch.float32) else torch.float32
        wavs, lengths = ops.preprocess_audio(audio_list, sample_rate, 15, 1, dtype=kdt, device=self.device, resample=resample)
        frames = [self._frames(int(n)) + 1 for n in lengths]
        pad = torch.ones(len(frames), max(frames, default=0), dtype=torch.bool)
        for i, f in enumerate(frames):
            pad[i, :f] = False
        return self.cast_data_dtype(wavs), pad.to(self.device)

    # ---- hipGraph replay of the extract_* calls (MI355X serving path; no reference counterpart) -----------------------
    def enable_graphs(self, on=True):
        """Capture each extract_* call into one hipGraph per input shape (one_peace_amd/graphs.py) and replay it: at batch
        1-8 the 40-layer forward is bound by the host's launch path.  Weights are captured by address: call again after
        loading new weights or moving the model."""
        self._graphs = {} if on else None
        return self

    def _run(self, tag, **kw):
        graphs = getattr(self, "_graphs", None)
        if graphs is None or not all(v.is_cuda for v in kw.values() if torch.is_tensor(v)):
            return self._eager(tag, **kw)
        if tag not in graphs:
            from ..graphs import GraphCache
            graphs[tag] = GraphCache(lambda _tag=tag, **k: self._eager(_tag, **k))
        return graphs[tag](**kw)

    def _eager(self, tag, **kw):
        if isinstance(self.model, OnePeaceClassifyModel):
            # hub_interface.py:206-225: the classify model is called without encoder_type and returns its logits.  (The reference's
            # extract_text_features forgets the `return` for this model type and yields None; the logits are returned here.)
            return self.model(**kw)
        if tag == "vl":
            tf, _, _ = self.model.encoder_wrapper(encoder_type="vl", **kw)
            return tf[:, 0, :]
        return self.model(encoder_type=tag, **kw)

    # ---- gallery search over extracted features (no reference counterpart) -------------------------------------------
    @torch.no_grad()
    def retrieve(self, query_features, gallery_features, k=10):
        """(scores fp32 [M, k], indices int64 [M, k]) of the k gallery rows with the largest dot product per query row: the
        extract_*_features outputs are L2-normalised, so this is cosine similarity.  ops.similarity_topk: on bf16 device features the
        [M, N] score matrix is never formed; exact ties rank the lower gallery index first."""
        from .. import ops
        return ops.similarity_topk(query_features, gallery_features, k)

    # ---- hub_interface.py:206-225 ---------------------------------------------------------------------------------
    @torch.no_grad()
    def extract_text_features(self, src_tokens):
        return self._run("text", src_tokens=src_tokens)

    @torch.no_grad()
    def extract_image_features(self, src_images):
        return self._run("image", src_images=self.cast_data_dtype(src_images))

    @torch.no_grad()
    def extract_audio_features(self, src_audios, audio_padding_masks):
        return self._run("audio", src_audios=self.cast_data_dtype(src_audios), audio_padding_masks=audio_padding_masks)

    @torch.no_grad()
    def extract_vl_features(self, src_images, src_tokens):
        return self._run("vl", src_tokens=src_tokens, src_images=self.cast_data_dtype(src_images))
