"""Generate tests/golden/pretrain_masks.pt from the UNMODIFIED reference mask code, run on CPU through oracle/ref_shim.py:
ImageTextPretrainDataset.__getitem__ and AudioTextPretrainDataset.__getitem__ (with a missing medium, which both accept), the
reference's collate_fn over their samples, and compute_block_mask_1d called directly.

    python tests/golden/make_pretrain_masks_golden.py      # needs the reference tree; writes pretrain_masks.pt

The dataset objects are made without their file-loading constructors and get a stub dictionary and bpe ("captions" are strings of
token ids) with a hand-made word-start table.  torchvision and soundfile, which the dataset modules import and this environment lacks,
are empty stand-in modules.  torch.randperm / randn / randint / multinomial are wrapped while the reference runs, and every recorded
choice is re-expressed as the keys and centres of this project's select(candidates, k, keys) rule:
  a chosen list [s0, s1, ...] (randperm, multinomial)  ->  key[s_j] = BIG - j, every other key 0
  randn values (ranked by argsort(descending))          ->  key = the value's rank, the largest value the largest key
  randint centres                                       ->  the centres themselves
The file holds only data: token ids, the table, keys, centres, and the reference's masks and preserve ids."""
import importlib
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402

BIG = 2 ** 31 - 1
VOCAB, PAD, EOS, BOS = 48, 1, 2, 0
SPEC = "[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512,2,2)] + [(512,2,2)]"


def word_start_table():
    """ids 0 ... 3 are the specials (word starts, as get_whole_word_mask has them); of the others every id that is not a multiple of 3
    starts a word, so runs of multiples of 3 are continuations."""
    return torch.tensor([1 if i < 4 or i % 3 else 0 for i in range(VOCAB)], dtype=torch.uint8)


class Dict:
    def bos(self):
        return BOS

    def eos(self):
        return EOS

    def pad(self):
        return PAD

    def encode_line(self, line, add_if_not_exist=False, append_eos=False):
        return torch.IntTensor([int(t) for t in line.split()])


class Bpe:
    def encode(self, text):
        return text


class Recorder:
    """Wraps the four torch functions the reference's mask code draws from; `calls` lists (name, arguments of interest, result)."""
    NAMES = ("randperm", "randn", "randint", "multinomial")

    def __enter__(self):
        self.calls, self.saved = [], {n: getattr(torch, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(torch, n, self._wrap(n))
        return self

    def _wrap(self, name):
        fn = self.saved[name]

        def wrapped(*a, **k):
            out = fn(*a, **k)
            self.calls.append((name, a, k, out.clone()))
            return out
        return wrapped

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(torch, n, fn)

    def take(self, name):
        for i, c in enumerate(self.calls):
            if c[0] == name:
                return self.calls.pop(i)
        raise AssertionError("no %s call recorded" % name)


def keys_of_list(n, chosen):
    k = torch.zeros(n, dtype=torch.int32)
    for j, s in enumerate(chosen):
        k[int(s)] = BIG - j
    return k


def keys_of_values(v):
    assert v.unique().numel() == v.numel()
    k = torch.empty(v.numel(), dtype=torch.int32)
    k[v.argsort()] = torch.arange(v.numel(), dtype=torch.int32)
    return k


def install_data_modules():
    R.install()
    root = os.path.join(R.REFERENCE_ROOT, "one_peace")
    for name in ("soundfile", "torchvision"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    tv = types.ModuleType("torchvision.transforms")
    tv.InterpolationMode = None
    sys.modules["torchvision.transforms"] = tv
    sys.modules["torchvision"].transforms = tv
    fd = R._shell("fairseq.data")
    fd.FairseqDataset = type("FairseqDataset", (), {})
    if "one_peace.utils" not in sys.modules:
        R._shell("one_peace.utils", os.path.join(root, "utils"))
    spec = importlib.util.spec_from_file_location("one_peace.data", os.path.join(root, "data", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(root, "data")])
    data = importlib.util.module_from_spec(spec)
    sys.modules["one_peace.data"] = data
    spec.loader.exec_module(data)
    R._shell("one_peace.data.pretrain_data", os.path.join(root, "data", "pretrain_data"))
    it = importlib.import_module("one_peace.data.pretrain_data.image_text_pretrain_dataset")
    at = importlib.import_module("one_peace.data.pretrain_data.audio_text_pretrain_dataset")
    du = importlib.import_module("one_peace.utils.data_utils")
    return data.collate_fn, it.ImageTextPretrainDataset, at.AudioTextPretrainDataset, du.compute_block_mask_1d


def bare(cls, table, **attrs):
    ds = cls.__new__(cls)
    d = Dict()
    ds.split, ds.dataset, ds.bpe, ds.dict = "train", None, Bpe(), d
    ds.bos, ds.eos, ds.pad = d.bos(), d.eos(), d.pad()
    ds._features_size_map = {}
    ds.max_src_length = 70
    ds.mask_whole_word = table
    for k, v in attrs.items():
        setattr(ds, k, v)
    return ds


def word_keys(rec, table, tokens):
    """The randperm of add_whole_word_mask -> keys over the caption's tokens."""
    starts = table[tokens.long()].nonzero().flatten()
    perm = rec.take("randperm")[3]
    assert perm.numel() == starts.numel()
    return keys_of_list(tokens.numel(), starts[perm])


CAPTIONS = [
    "4 5 7",                                     # every token its own word
    "5 6 9 12 7 3 8 10 15 18 21 4",              # words of 4, 2, 1, 5 tokens and a last word of one
    "6 9 5 7 12",                                # the first token starts no word; the last word runs to the end
    "5 6 9 12 15 18 21 24 27 30",                # ONE word (W = 1)
    "7 8 10 11 13 14 16 17 19 20 22 23 25 26 28 29 31 32 34 35 37 38 40 41 43 44 46 47 4 5",   # 30 one-token words
    "5 6 7 9 8 12 15 10 3 11 13 18 14 16 21 24 27 17",
    " ".join(str(4 + (i * 7) % 44) for i in range(70)),   # max_src_length tokens
    " ".join(str(4 + (i * 5) % 44) for i in range(90)),   # cut to 70 by encode_text
]


def image_text_cases(collate_fn, Cls, table):
    out = []
    for size, ratios in ((256, (0.15, 0.75, 0.4, 0.6875)), (64, (0.15, 0.75, 0.4, 0.6875)), (112, (0.3, 0.5, 0.25, 0.8))):
        ds = bare(Cls, table, text_mask_ratio=ratios[0], image_mask_ratio=ratios[1], vl_text_mask_ratio=ratios[2], vl_image_mask_ratio=ratios[3],
                  num_patches=(size // 16) ** 2, patch_image_size=size)
        N = ds.num_patches
        samples, keys = [], []
        for i, cap in enumerate(CAPTIONS):
            if i == 3:  # W = 1 masks the whole caption: no unmasked token is left for the vl pass (audio-text has no such pass)
                continue
            torch.manual_seed(1000 * size + i)
            with Recorder() as rec:
                ex = ds.__getitem__(i, item_tuple=(i, None, cap))
            tokens = ex["source_text"][:-1]
            n = tokens.numel()
            ka = word_keys(rec, table, tokens)
            kb = keys_of_values(rec.take("randn")[3])
            assert kb.numel() == n
            k2 = int(n * ratios[2])
            assert k2 <= int((~ex["text_mask_indices"][1:-1]).sum()), "the reference's argsort is unspecified here: pick another caption"
            assert tuple(rec.take("randn")[3].shape) == (size, size)  # the stand-in image
            pa = keys_of_list(N, rec.take("randperm")[3])
            pb = keys_of_values(rec.take("randn")[3])
            assert not rec.calls and pb.numel() == N
            del ex["source_image"]
            samples.append(ex)
            keys.append({"text_a": ka, "text_b": kb, "image_a": pa, "image_b": pb})
        batch = collate_fn([dict(s, source_image=torch.zeros(1)) for s in samples], pad_idx=PAD)["net_input"]
        del batch["src_images"], batch["src_audios"], batch["audio_padding_masks"]
        out.append({"patch_image_size": size, "ratios": ratios, "samples": samples, "keys": keys, "batch": batch})
    return out


def audio_text_cases(collate_fn, Cls, table):
    ds = bare(Cls, table, max_duration=15, feature_encoder_spec=eval(SPEC), audio_mask_ratio=0.55, al_text_mask_ratio=0.4,
              al_audio_mask_ratio=0.45, audio_mask_prob_adjust=0.1, audio_mask_length=5)
    samples, keys = [], []
    for i, cap in enumerate(CAPTIONS):
        torch.manual_seed(77 + i)
        with Recorder() as rec:
            ex = ds.__getitem__(i, item_tuple=(i, None, cap, None))
        tokens = ex["source_text"][:-1]
        ka = word_keys(rec, table, tokens)
        assert tuple(rec.take("randn")[3].shape) == (16000,)  # the stand-in waveform
        T = ex["audio_padding_mask"].numel() - 1
        entry = {"text_a": ka, "frames": T}
        for name in ("audio", "al_audio"):
            entry[name + "_centers"] = rec.take("randint")[3].flatten().to(torch.int32)
            final = ex[name + "_mask_indices"][1:]
            # the multinomial call of this mask, if it made one: it comes before the next mask's randint
            nxt = [c[0] for c in rec.calls]
            has = nxt and nxt[0] == "multinomial"
            entry[name + "_keys"] = keys_of_list(T, rec.take("multinomial")[3].flatten()) if has else torch.zeros(T, dtype=torch.int32)
            assert final.numel() == T
        assert not rec.calls
        del ex["source_audio"]
        samples.append(ex)
        keys.append(entry)
    batch = collate_fn([dict(s, source_audio=torch.zeros(1)) for s in samples], pad_idx=PAD)["net_input"]
    del batch["src_images"], batch["src_audios"]
    return {"samples": samples, "keys": keys, "batch": batch,
            "args": {"audio_mask_ratio": 0.55, "al_text_mask_ratio": 0.4, "al_audio_mask_ratio": 0.45, "audio_mask_prob_adjust": 0.1,
                     "audio_mask_length": 5}}


def block_cases(compute_block_mask_1d):
    out = []
    seed = 0
    for T in (7, 49, 50, 249, 749):
        for p in (0.55, 0.45):
            for _ in range(4):
                seed += 1
                torch.manual_seed(seed)
                with Recorder() as rec:
                    mask = compute_block_mask_1d(shape=(1, T), mask_prob=p, mask_length=5, mask_prob_adjust=0.1).squeeze(0).bool()
                centers = rec.take("randint")[3].flatten().to(torch.int32)
                keys = keys_of_list(T, rec.take("multinomial")[3].flatten()) if rec.calls else torch.zeros(T, dtype=torch.int32)
                assert not rec.calls
                out.append({"T": T, "p": p, "length": 5, "adjust": 0.1, "centers": centers, "keys": keys, "mask": mask})
    return out


def main():
    collate_fn, ImageText, AudioText, compute_block_mask_1d = install_data_modules()
    table = word_start_table()
    out = {"table": table, "pad": PAD, "eos": EOS, "captions": CAPTIONS,
           "image_text": image_text_cases(collate_fn, ImageText, table),
           "audio_text": audio_text_cases(collate_fn, AudioText, table),
           "blocks": block_cases(compute_block_mask_1d)}
    path = os.path.join(HERE, "pretrain_masks.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
