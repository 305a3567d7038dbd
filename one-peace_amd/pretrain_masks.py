"""The mask tensors of a pretraining batch, made on the batch's device (csrc/masks.hip through ops.patch_masks / word_masks /
block_masks): what the reference's datasets make per sample on the host
(one_peace/data/pretrain_data/image_text_pretrain_dataset.py:61-139, audio_text_pretrain_dataset.py:43-116,
one_peace/utils/data_utils.py:110-231) and collate_fn (one_peace/data/__init__.py:50-81) pads into a batch.

Every random choice of the reference is a uniform choice of k items out of a candidate set; here it is select(candidates, k, keys) with
int32 keys drawn by ONE torch.randint call per batch on the batch's device (`generator`, or that device's default generator): the k
candidates first by (key descending, index ascending).  The rules are the reference's, its random stream is not reproduced; and as the
CPU and the device generators of torch differ, the same seed gives different masks on the two, by design.  For given keys the CPU and the
device routes give the same bits."""
import torch

from . import ops

KEY_HIGH = 2 ** 31 - 1  # keys are drawn from [0, 2^31 - 1)


def whole_word_table(dictionary, bpe):
    """get_whole_word_mask (one_peace/utils/data_utils.py:88-107): uint8 [len(dictionary)], 1 where the entry begins a word: the special
    symbols, 'madeupword...' entries, entries the bpe says begin a word or cannot decode.  None without a bpe, as there."""
    if bpe is None:
        return None

    def begins(i):
        if i < dictionary.nspecial:
            return True
        tok = dictionary[i]
        if tok.startswith("madeupword"):
            return True
        try:
            return bool(bpe.is_beginning_of_word(tok))
        except ValueError:
            return True
    return torch.tensor([begins(i) for i in range(len(dictionary))], dtype=torch.uint8)


def _draw(total, device, generator):
    if generator is not None and torch.device(generator.device).type != torch.device(device).type:
        raise ValueError("pretrain masks: the generator lives on %s, the batch on %s" % (generator.device, device))
    return torch.randint(0, KEY_HIGH, (total,), dtype=torch.int32, device=device, generator=generator)


def _carve(flat, shapes):
    out, at = [], 0
    for shape in shapes:
        n = shape[0] * shape[1]
        out.append(flat[at:at + n].view(shape))
        at += n
    return out


class _Masks:
    def __init__(self, word_start, pad):
        if not torch.is_tensor(word_start) or word_start.dtype != torch.uint8 or word_start.dim() != 1:
            raise ValueError("word_start must be a uint8 [vocab] tensor (whole_word_table)")
        self.word_start, self.pad = word_start, int(pad)
        self._tables = {}

    def _table(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = self.word_start.to(device).contiguous()
        return self._tables[key]


class ImageTextPretrainMasks(_Masks):
    """The eight mask tensors ImageTextPretrainDataset adds to a batch: {text, image, vl_text, vl_image}_{mask_indices, preserve_ids}.
    The defaults are that dataset's.  The vl image mask contains every patch the image mask leaves visible, and the vl text mask is
    drawn among the tokens the text mask leaves visible, as in the reference.

    __call__(net_input, frames=None, generator=None, width=None) returns a copy of net_input with those keys, on the device of
    net_input["src_tokens"] (int64 [B, L]: tokens, eos, pad).  width: see ops.word_masks -- None reads the widths of the two text id
    tensors back from the device once; an int or a pair is an upper bound without a synchronisation.  `frames` is unused here."""

    def __init__(self, word_start, patch_image_size=256, text_mask_ratio=0.15, image_mask_ratio=0.75, vl_text_mask_ratio=0.4,
                 vl_image_mask_ratio=0.6875, pad=1):
        super().__init__(word_start, pad)
        self.num_patches = (patch_image_size // 16) ** 2
        self.text_mask_ratio, self.vl_text_mask_ratio = text_mask_ratio, vl_text_mask_ratio
        N = self.num_patches
        self.mask_patches = int(N * image_mask_ratio)                                    # image_text_pretrain_dataset.py:85
        self.vl_extra = int(N * vl_image_mask_ratio) - (N - self.mask_patches)           # :89, :92
        if N < 1 or not 0 <= self.vl_extra <= self.mask_patches <= N:
            raise ValueError("ImageTextPretrainMasks: %d patches, %d masked, %d of them masked again in the vl pass: need "
                             "0 <= extra <= masked <= patches" % (N, self.mask_patches, self.vl_extra))

    def draw_keys(self, B, L, device, generator=None):
        """The keys of one batch, ONE torch.randint call: {"text_a", "text_b": int32 [B, L], "image_a", "image_b": int32 [B, N]}."""
        N = self.num_patches
        return dict(zip(("text_a", "text_b", "image_a", "image_b"),
                        _carve(_draw(2 * B * (L + N), device, generator), [(B, L), (B, L), (B, N), (B, N)])))

    def apply(self, net_input, keys, width=None):
        """The masks for given keys (draw_keys): a pure function of the tokens and the keys."""
        tok = net_input["src_tokens"]
        out = dict(net_input)
        m, ids, vm, vids, _ = ops.word_masks(tok, self._table(tok.device), keys["text_a"], self.text_mask_ratio, keys["text_b"],
                                             self.vl_text_mask_ratio, self.pad, width)
        out["text_mask_indices"], out["text_preserve_ids"], out["vl_text_mask_indices"], out["vl_text_preserve_ids"] = m, ids, vm, vids
        m, ids, vm, vids = ops.patch_masks(keys["image_a"], keys["image_b"], self.mask_patches, self.vl_extra)
        out["image_mask_indices"], out["image_preserve_ids"], out["vl_image_mask_indices"], out["vl_image_preserve_ids"] = m, ids, vm, vids
        return out

    def __call__(self, net_input, frames=None, generator=None, width=None):
        tok = net_input["src_tokens"]
        return self.apply(net_input, self.draw_keys(tok.shape[0], tok.shape[1], tok.device, generator), width)


class AudioTextPretrainMasks(_Masks):
    """The six mask tensors AudioTextPretrainDataset adds to a batch: {audio, al_text, al_audio}_{mask_indices, preserve_ids}.  The
    defaults are that dataset's.  The two audio masks are compute_block_mask_1d's default path (ops.block_masks) at audio_mask_ratio and
    al_audio_mask_ratio; the text mask is the whole-word mask at al_text_mask_ratio.

    __call__(net_input, frames=None, generator=None, width=None): `frames` is a host sequence of the clips' frame counts T_b (what
    frame_count gives for each clip's samples); absent, it is taken from net_input["audio_padding_masks"] (bool [B, Tmax + 1], True =
    padding, position 0 = CLS) with ONE device-to-host read.  Block centres are (key * T_b) >> 31 in int64, never a float product.
    width: the bound of the text ids, as in ops.word_masks; the audio ids have their host-known widths."""

    def __init__(self, word_start, audio_mask_ratio=0.55, al_text_mask_ratio=0.4, al_audio_mask_ratio=0.45, audio_mask_prob_adjust=0.1,
                 audio_mask_length=5, feature_encoder_spec="[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512,2,2)] + [(512,2,2)]", pad=1):
        super().__init__(word_start, pad)
        self.audio_mask_ratio, self.al_text_mask_ratio, self.al_audio_mask_ratio = audio_mask_ratio, al_text_mask_ratio, al_audio_mask_ratio
        self.audio_mask_prob_adjust, self.audio_mask_length = audio_mask_prob_adjust, int(audio_mask_length)
        self.feature_encoder_spec = eval(feature_encoder_spec) if isinstance(feature_encoder_spec, str) else list(feature_encoder_spec)

    def frame_count(self, samples):
        """BaseDataset._get_mask_indices_dims: the frames the feature encoder makes of `samples` waveform samples."""
        n = int(samples)
        for _, kernel, stride in self.feature_encoder_spec:
            n = (n - (kernel - 1) - 1) // stride + 1
        return n

    def frames_of(self, net_input, frames=None):
        """(the clips' frame counts as a list of ints, Tmax)."""
        pad_mask = net_input.get("audio_padding_masks")
        if frames is None:
            if pad_mask is None:
                raise ValueError("AudioTextPretrainMasks: need `frames` or net_input['audio_padding_masks']")
            frames = ((~pad_mask).sum(1) - 1).clamp(min=0).tolist()  # the one device-to-host read
        frames = [int(t) for t in frames]
        if len(frames) != net_input["src_tokens"].shape[0]:
            raise ValueError("AudioTextPretrainMasks: %d frame counts for %d samples" % (len(frames), net_input["src_tokens"].shape[0]))
        return frames, (pad_mask.shape[1] - 1 if pad_mask is not None else max(frames + [1]))

    def draw_keys(self, B, L, frames, Tmax, device, generator=None):
        """The keys of one batch, ONE torch.randint call: {"text_a": int32 [B, L]; "audio_centers", "al_audio_centers": int32 [B, Kmax],
        centre j of clip b = (key * T_b) >> 31 in int64; "audio_keys", "al_audio_keys": int32 [B, Tmax]}."""
        Kmax = [max([ops.block_counts(t, p, self.audio_mask_length, self.audio_mask_prob_adjust)[0] for t in frames] + [1])
                for p in (self.audio_mask_ratio, self.al_audio_mask_ratio)]
        ta, c0, k0, c1, k1 = _carve(_draw(B * (L + 2 * Tmax + Kmax[0] + Kmax[1]), device, generator),
                                    [(B, L), (B, Kmax[0]), (B, Tmax), (B, Kmax[1]), (B, Tmax)])
        T = torch.tensor(frames, dtype=torch.int64).to(device).view(B, 1)
        return {"text_a": ta, "audio_centers": ((c0.long() * T) >> 31).to(torch.int32), "audio_keys": k0,
                "al_audio_centers": ((c1.long() * T) >> 31).to(torch.int32), "al_audio_keys": k1}

    def apply(self, net_input, keys, frames, width=None):
        """The masks for given keys (draw_keys) and frame counts: a pure function of the tokens, the keys and the counts."""
        tok = net_input["src_tokens"]
        out = dict(net_input)
        m, ids, _, _, _ = ops.word_masks(tok, self._table(tok.device), keys["text_a"], self.al_text_mask_ratio, pad=self.pad, width=width)
        out["al_text_mask_indices"], out["al_text_preserve_ids"] = m, ids
        for name, p in (("audio", self.audio_mask_ratio), ("al_audio", self.al_audio_mask_ratio)):
            m, ids = ops.block_masks(frames, keys[name + "_centers"], keys[name + "_keys"], p, self.audio_mask_length, self.audio_mask_prob_adjust)
            out[name + "_mask_indices"], out[name + "_preserve_ids"] = m, ids
        return out

    def __call__(self, net_input, frames=None, generator=None, width=None):
        tok = net_input["src_tokens"]
        frames, Tmax = self.frames_of(net_input, frames)
        return self.apply(net_input, self.draw_keys(tok.shape[0], tok.shape[1], frames, Tmax, tok.device, generator), frames, width)
