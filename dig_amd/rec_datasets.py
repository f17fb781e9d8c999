"""Labelled data sources of recognition fine-tuning and evaluation, and the loader that puts their batches on the device.

The reference's `ImageLmdb` (dataset/dataset_lmdb.py) decodes a crop, augments and resizes it and encodes its word, per sample, in a
dataloader worker.  Here a dataset returns `(uint8 HxWx3 crop, word)` and nothing else; `DeviceBatches` runs `FinetuneBatchTransform` (resize /
ABINet / seqCLR views) and `LabelEncoder` on whole batches on the MI355X and yields the `(images, targets, tgt_lens)` triple that
`engine_for_finetuning.train_one_epoch` and `evaluate` consume.

    image_lmdb   the reference layout (`num-samples`, `image-%09d`, `label-%09d`), read through the `lmdb` module where it is installed
    image_list   a directory with `gt.txt`, one `relative/path<TAB>word` per line, decoded with Pillow
    synthetic    N seeded random words drawn with Pillow's built-in font, held in memory

Every dataset carries `classes / class_to_idx / idx_to_class` (dataset_lmdb.py:70-72) and keeps the reference's two substitution rules
(:173-187): an image that does not decode, or a word with `len(word) + 1 >= max_len`, is replaced by the next sample.  The reference's
`self[index + 1]` runs after `index += 1`, so it skips one sample and can run past the end of the database; here the substitute is the
sample right behind the refused one, wrapping at the end.  `num_samples` follows :27-28: a value <= 1 is a fraction of the source."""
import math
import os

import numpy as np
import torch

from .datasets import FinetuneBatchTransform, LabelEncoder


def _cap(n, num_samples):
    """dataset_lmdb.py:27-28."""
    num_samples = num_samples if num_samples > 1 else int(n * num_samples)
    return int(min(n, num_samples))


def _decode(buf_or_path):
    """RGB uint8 crop of an encoded image (bytes or a path); OSError (Pillow's IOError) when it does not decode."""
    import io
    from PIL import Image
    src = io.BytesIO(buf_or_path) if isinstance(buf_or_path, (bytes, bytearray, memoryview)) else buf_or_path
    with Image.open(src) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class LabelledCrops(torch.utils.data.Dataset):
    """Base of the three sources: vocabulary, length cap and the substitution rules around `_read(i) -> (crop, word)`."""

    def __init__(self, voc_type, max_len, n_source, num_samples=math.inf):
        enc = LabelEncoder(voc_type, max_len, "cpu")                     # (the vocabulary only: nothing is encoded here)
        self.voc_type, self.max_len = voc_type, int(max_len)
        self.classes, self.class_to_idx, self.idx_to_class = enc.classes, enc.class_to_idx, enc.idx_to_class
        self.use_lowercase = enc.use_lowercase
        self.nSamples = _cap(n_source, num_samples)

    def __len__(self):
        return self.nSamples

    def _read(self, i):
        raise NotImplementedError

    def __getitem__(self, index):
        if not 0 <= index < len(self):
            raise IndexError(index)
        for k in range(len(self)):
            i = (index + k) % len(self)
            try:
                crop, word = self._read(i)
            except OSError:
                print("Corrupted image for %d" % (i + 1))
                continue
            if self.use_lowercase:
                word = word.lower()
            if len(word) + 1 >= self.max_len:
                continue
            return crop, word
        raise RuntimeError("no sample of the dataset decodes with a word shorter than max_len - 1")


class ImageLmdb(LabelledCrops):
    """The reference's LMDB layout (dataset_lmdb.py:23-28,160-183).  The `lmdb` module is imported when the first dataset is built."""

    def __init__(self, root, voc_type, max_len, num_samples=math.inf):
        self.root = root
        n = int(self._txn().get(b"num-samples"))
        super().__init__(voc_type, max_len, n, num_samples)

    def _txn(self):
        txn = getattr(self, "txn", None)
        if txn is None:
            try:
                import lmdb
            except ImportError as e:
                raise ImportError("--data_set image_lmdb reads through the `lmdb` module, which is not installed.  Without it: --data_set image_list "
                                  "(a directory with gt.txt: one `relative/path<TAB>word` per line), or --data_path synthetic") from e
            self.env = lmdb.open(self.root, max_readers=32, readonly=True)
            txn = self.txn = self.env.begin()
        return txn

    def __getstate__(self):                                               # a dataloader worker opens its own environment
        return {k: v for k, v in self.__dict__.items() if k not in ("env", "txn")}

    def _read(self, i):
        txn = self._txn()
        buf = txn.get(b"image-%09d" % (i + 1))
        if buf is None:
            raise OSError("no image-%09d" % (i + 1))
        return _decode(bytes(buf)), txn.get(b"label-%09d" % (i + 1)).decode()


class ImageList(LabelledCrops):
    """A directory with `gt.txt`: `relative/path<TAB>word` per line (a word may be empty, or hold further tabs)."""

    def __init__(self, root, voc_type, max_len, num_samples=math.inf):
        self.root = root
        gt = os.path.join(root, "gt.txt")
        if not os.path.isfile(gt):
            raise FileNotFoundError(f"{gt}: an image_list dataset is a directory with gt.txt (`relative/path<TAB>word` per line)")
        with open(gt, encoding="utf-8") as f:
            lines = [l.rstrip("\r\n") for l in f]
        self.items = [tuple(l.split("\t", 1)) if "\t" in l else (l, "") for l in lines if l]
        super().__init__(voc_type, max_len, len(self.items), num_samples)

    def _read(self, i):
        path, word = self.items[i]
        return _decode(os.path.join(self.root, path)), word


class SyntheticWords(LabelledCrops):
    """`n` random words of 1 .. max_len - 2 characters over the vocabulary, drawn with Pillow's built-in default font on crops of
    24-64 x 60-320 pixels.  Sample i depends on (seed, i) alone, so every process sees the same data."""
    H, W = (24, 64), (60, 320)

    def __init__(self, n, voc_type, max_len, seed=0, num_samples=math.inf):
        if max_len < 3:
            raise ValueError("synthetic words need max_len >= 3")
        super().__init__(voc_type, max_len, int(n), num_samples)
        self.seed = int(seed)
        chars = self.classes[:-3]
        if self.use_lowercase:
            chars = [c for c in chars if c == c.lower()]
        self.samples = [self._make(i, chars) for i in range(self.nSamples)]

    def _make(self, i, chars):
        from PIL import Image, ImageDraw, ImageFont
        rng = np.random.RandomState([self.seed & 0x7fffffff, i])
        word = "".join(chars[k] for k in rng.randint(0, len(chars), size=rng.randint(1, self.max_len - 1)))
        h, w = rng.randint(self.H[0], self.H[1] + 1), rng.randint(self.W[0], self.W[1] + 1)
        bg = rng.randint(128, 256, size=3)
        fg = rng.randint(0, 96, size=3)
        font = ImageFont.load_default()
        box = ImageDraw.Draw(Image.new("RGB", (1, 1))).textbbox((0, 0), word, font=font)
        tile = Image.new("RGB", (max(1, box[2] - box[0]) + 4, max(1, box[3] - box[1]) + 4), tuple(int(v) for v in bg))
        ImageDraw.Draw(tile).text((2 - box[0], 2 - box[1]), word, fill=tuple(int(v) for v in fg), font=font)
        return np.asarray(tile.resize((w, h), Image.BILINEAR), dtype=np.uint8), word

    def _read(self, i):
        return self.samples[i]


class ConcatDataset(torch.utils.data.ConcatDataset):
    """dataset/concatdatasets.py:35-37: several roots as one dataset with the vocabulary of the first."""

    def __init__(self, datasets):
        super().__init__(datasets)
        self.classes, self.class_to_idx, self.idx_to_class = datasets[0].classes, datasets[0].class_to_idx, datasets[0].idx_to_class


def _roots(path):
    return [p for p in ([path] if isinstance(path, str) else list(path or [])) if p]


def build_dataset(is_train, args):
    """dataset/datasets.py:67-123 for the labelled sources: (dataset, nb_classes) from `--data_path` (training) or `--eval_data_path`.
    `synthetic` as a path selects SyntheticWords whatever `--data_set` says (the evaluation set draws from seed + 1); under image_lmdb a
    root that holds `gt.txt` and no `data.mdb` is read as an image_list, so the README commands run as written on either."""
    roots = _roots(args.data_path if is_train else args.eval_data_path)
    if not roots:
        raise SystemExit("--data_path is empty" if is_train else "--eval_data_path is not given (or pass --disable_eval_during_finetuning)")
    cap = args.num_samples if is_train else math.inf
    out = []
    for root in roots:
        if root == "synthetic":
            n = int(getattr(args, "synthetic", 0) or 0)
            if n <= 0:
                raise SystemExit("--data_path synthetic needs --synthetic N")
            out.append(SyntheticWords(n, args.voc_type, args.max_len, seed=args.seed + (0 if is_train else 1), num_samples=cap))
        elif args.data_set == "image_list" or (os.path.isfile(os.path.join(root, "gt.txt")) and not os.path.isfile(os.path.join(root, "data.mdb"))):
            out.append(ImageList(root, args.voc_type, args.max_len, cap))
        elif args.data_set == "image_lmdb":
            out.append(ImageLmdb(root, args.voc_type, args.max_len, cap))
        else:
            raise NotImplementedError(f"--data_set {args.data_set}")
    dataset = out[0] if len(out) == 1 else ConcatDataset(out)
    nb_classes = len(dataset.classes)
    if nb_classes != args.nb_classes:
        raise SystemExit(f"--nb_classes {args.nb_classes}, but --voc_type {args.voc_type} has {nb_classes} classes")
    print("Number of the class = %d" % args.nb_classes)
    return dataset, nb_classes


def collate(samples):
    """[(crop, word)] -> (list of crops, list of words): crops differ in size, so nothing is stacked on the host."""
    return [s[0] for s in samples], [s[1] for s in samples]


def make_loader(dataset, args, is_train, rank=0, world=1):
    """The samplers and loaders of run_class_finetuning.py:291-334: training shuffles through DistributedSampler and drops the last partial
    batch; evaluation takes batches of int(1.5 * batch_size), in order (or sharded under --dist_eval), and keeps it."""
    if is_train:
        sampler = torch.utils.data.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True)
    elif getattr(args, "dist_eval", False):
        if len(dataset) % world != 0:
            print('Warning: Enabling distributed evaluation with an eval dataset not divisible by process number. '
                  'This will slightly alter validation results as extra duplicate entries are added to achieve '
                  'equal num of samples per-process.')
        sampler = torch.utils.data.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=False)
    else:
        sampler = torch.utils.data.SequentialSampler(dataset)
    return torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=args.batch_size if is_train else int(1.5 * args.batch_size),
                                       num_workers=args.num_workers, drop_last=is_train, collate_fn=collate)


class DeviceBatches:
    """A loader of `(crops, words)` batches as the loader the engine iterates: `(images, targets, tgt_lens)` on the device, through
    `transform` (a FinetuneBatchTransform) and `encoder` (a LabelEncoder)."""

    def __init__(self, loader, transform, encoder):
        self.loader, self.transform, self.encoder = loader, transform, encoder

    @property
    def dataset(self):
        return self.loader.dataset

    @property
    def sampler(self):
        return self.loader.sampler

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for crops, words in self.loader:
            targets, lens = self.encoder(words)
            yield self.transform(crops), targets, lens


def device_loader(dataset, args, is_train, device, seed=0, rank=0, world=1):
    """make_loader + the device-side transform and label encoder of `args`."""
    return DeviceBatches(make_loader(dataset, args, is_train, rank, world), FinetuneBatchTransform(args, is_train, seed=seed, device=device),
                         LabelEncoder(args.voc_type, args.max_len, device))
