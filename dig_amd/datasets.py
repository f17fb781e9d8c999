"""Device-side input transform: the reference's `DataAugmentationForMAE` (dataset/datasets.py:27-52) with the
resize / ToTensor / Normalize and the mask generator running on the MI355X instead of in dataloader workers.

The reference pipeline per sample (dataset/dataset_image.py:128-160): decode the crop to an RGB PIL image, optionally run
the imgaug augmentor on it (CPU, stays on the host), then `transform(img) -> (tensor [3,32,128], mask [num_view, 256])`.
Here the dataloader hands over the *decoded uint8 crops* (any size); `GpuBatchTransform` packs them into one pinned
buffer, uploads it once (H x W x 3 bytes per crop instead of 3 x 32 x 128 x 4 after resize -- usually less), and one kernel
per view produces the normalised fp32 batch bit-exactly as Pillow + torchvision would; masks are drawn on the device.

    tf = GpuBatchTransform(args)                       # args.input_h/input_w/window_size/mask_ratio/num_view as in the reference
    images, aug_images, masks = tf(crops, aug_crops)   # lists of HxWx3 uint8 arrays -> the `batch` triple of train_one_epoch

With `key_view_aug="seqclr"` and no `aug_crops`, the second view is the reference's augmented key view (seqCLR ops + ColorJitter +
RandomGrayscale), drawn and applied on the device from the first view's upload (dig_amd/augment.py).

For fine-tuning, `FinetuneBatchTransform` is the image side and `LabelEncoder` the label side: words -> target rows and lengths, on the device
(`dig_encode_labels`); dig_amd/rec_datasets.py puts both behind a loader.
"""
import ctypes
import string

import numpy as np
import torch

from . import _lib as L
from .augment import AbiAugment, KeyViewAugment, PackedCrops, pack_crops


class RandomMaskingGenerator:
    """masking_generator.py:12-49 on the device: `__call__(n)` returns [n, num_view, num_patches] uint8 with exactly
    `num_mask` ones per view.  The reference draws from numpy's global Mersenne Twister inside dataloader workers; this
    generator keeps the distribution (uniform over subsets of that size) with its own counter-based stream (Philox4x32-10,
    key = seed, counter = (row, patch, call index)), so a run is reproducible from (seed, step) on any number of ranks."""

    def __init__(self, input_size, mask_ratio, aug_ratio=0., num_view=1, seed=0, device="cuda"):
        if not isinstance(input_size, tuple):
            input_size = (input_size,) * 2
        self.height, self.width = input_size
        self.num_patches = self.height * self.width
        self.num_mask = int(mask_ratio * self.num_patches)
        self.num_aug = int(self.num_mask * aug_ratio)
        self.num_view = num_view
        self.seed, self.step, self.device = int(seed), 0, torch.device(device)

    def __repr__(self):
        return "Mask: total patches {}, mask patches {}".format(self.num_patches, self.num_mask)

    def __call__(self, n=1):
        rows = n * self.num_view
        mask = torch.empty((rows, self.num_patches), device=self.device, dtype=torch.uint8)
        L.call("dig_random_masks", L.ptr(mask), rows, self.num_patches, self.num_mask, ctypes.c_ulonglong(self.seed),
               ctypes.c_uint(self.step & 0xFFFFFFFF), L.stream())
        self.step += 1
        return mask.view(n, self.num_view, self.num_patches)


def resize_normalize(crops, out_h=32, out_w=128, mean=0.5, std=0.5, device="cuda"):
    """List of HxWx3 uint8 numpy arrays (or a PackedCrops upload of them) -> fp32 [n, 3, out_h, out_w] on `device`:
    Normalize(mean, std)(ToTensor(Resize((out_h, out_w), interpolation=BICUBIC)(PIL crop)))  (datasets.py:31-37)."""
    pk = crops if isinstance(crops, PackedCrops) else pack_crops(crops, device)
    out = torch.empty((pk.n, 3, out_h, out_w), device=pk.data.device, dtype=torch.float32)
    L.call("dig_resize_bicubic_normalize_u8", L.ptr(pk.data), L.ptr(pk.offsets), L.ptr(pk.heights), L.ptr(pk.widths), pk.n, L.ptr(out), out_h,
           out_w, ctypes.c_float(mean), ctypes.c_float(std), pk.max_h, pk.max_w, L.stream())
    return out


class GpuBatchTransform:
    """Batch form of DataAugmentationForMAE.__call__ (datasets.py:41-42): (crops, aug_crops) -> (images, aug_images, masks).

    key_view_aug="seqclr": without explicit `aug_crops` the second view is the reference's augmented key view (dataset_image.py:39-50,
    88-120,145-149), built on the device from the same upload as the first view (dig_amd/augment.py).  Explicit `aug_crops`, or
    key_view_aug=None, give the plain transform of what is passed (None -> no second view)."""

    def __init__(self, args, seed=0, device="cuda", key_view_aug=None):
        self.h, self.w = args.input_h, args.input_w
        self.device = device
        self.masked_position_generator = RandomMaskingGenerator(args.window_size, args.mask_ratio, num_view=args.num_view,
                                                                seed=seed, device=device)
        if key_view_aug not in (None, "seqclr"):
            raise ValueError(f"key_view_aug must be None or 'seqclr', not {key_view_aug!r}")
        self.key_view = KeyViewAugment(seed, device, self.h, self.w) if key_view_aug == "seqclr" else None

    def __call__(self, crops, aug_crops=None):
        packed = pack_crops(crops, self.device)
        images = resize_normalize(packed, self.h, self.w)
        if aug_crops is not None:
            aug = resize_normalize(aug_crops, self.h, self.w, device=self.device)
        else:
            aug = self.key_view(packed) if self.key_view is not None else None
        masks = self.masked_position_generator(len(crops))
        return images, aug, masks


class FinetuneBatchTransform:
    """The fine-tune input transform for whole batches, with build_dataset's rule (dataset/datasets.py:68,110-116 of the reference):
    crops (a list of HxWx3 uint8 arrays or a PackedCrops) -> fp32 [n, 3, input_h, input_w] on the device.

      not training, or num_view <= 1      resize_normalize (the reference's eval / single-view transform)
      num_view > 1 and use_abi_aug        AbiAugment (CVGeometry, CVDeterioration, CVColorJitter, Resize, Normalize)
      num_view > 1 without it             KeyViewAugment (ImageLmdb.sequential_aug + aug_transformer = the MoCo key view)

    Labels stay with the caller."""

    def __init__(self, args, is_train, seed=0, device="cuda"):
        self.h, self.w, self.device = args.input_h, args.input_w, device
        if not is_train or getattr(args, "num_view", 1) <= 1:
            self.kind, self.aug = "resize", None
        elif getattr(args, "use_abi_aug", False):
            self.kind, self.aug = "abi", AbiAugment(seed, device, self.h, self.w)
        else:
            self.kind, self.aug = "keyview", KeyViewAugment(seed, device, self.h, self.w)

    def __call__(self, crops):
        packed = crops if isinstance(crops, PackedCrops) else pack_crops(crops, self.device)
        if self.aug is None:
            return resize_normalize(packed, self.h, self.w)
        return self.aug(packed)


VOC_TYPES = ("LOWERCASE", "ALLCASES", "ALLCASES_SYMBOLS")


def find_classes(voc_type, EOS="EOS", PADDING="PADDING", UNKNOWN="UNKNOWN"):
    """ImageLmdb._find_classes (dataset/dataset_lmdb.py:75-97): the character list of a vocabulary type plus the three special classes."""
    if voc_type == "LOWERCASE":
        voc = list(string.digits + string.ascii_lowercase + '!"#$%&\'()*+,-./:;<=>?@[\\]^_`{|}~')
    elif voc_type == "ALLCASES":
        voc = list(string.digits + string.ascii_letters)
    elif voc_type == "ALLCASES_SYMBOLS":
        voc = list(string.printable[:-6])
    else:
        raise KeyError('voc_type must be one of "LOWERCASE", "ALLCASES", "ALLCASES_SYMBOLS"')
    return voc + [EOS, PADDING, UNKNOWN]


def encode_code_points(rows, class_of, eos, padding, unknown, max_len, device):
    """`dig_encode_labels` on a batch of words given as sequences of code points: (labels int64 [B, max_len], lens int64 [B]) on `device`.
    class_of: int32 [128] on `device`.  chars and offsets travel in one (pinned) buffer, offsets first.  Every row must fit:
    len(row) + 1 <= max_len (the callers check; the kernel clamps)."""
    B = len(rows)
    dev = torch.device(device)
    labels = torch.empty((B, max_len), device=dev, dtype=torch.int64)
    lens = torch.empty(B, device=dev, dtype=torch.int64)
    if B == 0:                                                                    # (empty tensors have no address to hand over)
        return labels, lens
    offs = np.zeros(B + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    host = torch.empty(B + 1 + max(int(offs[-1]), 1), dtype=torch.int32)           # (one spare cell: `chars` is never a null pointer)
    if dev.type == "cuda":
        host = host.pin_memory()
    flat = host.numpy()
    flat[:B + 1] = offs
    flat[B + 1:B + 1 + int(offs[-1])] = np.fromiter((c for r in rows for c in r), dtype=np.int32, count=int(offs[-1]))
    up = host.to(dev, non_blocking=True)
    L.call("dig_encode_labels", L.ptr(up[B + 1:]), L.ptr(up), L.ptr(class_of), eos, padding, unknown, max_len, B, L.ptr(labels), L.ptr(lens), L.stream())
    return labels, lens


class LabelEncoder:
    """Words -> the `[B, max_len]` target rows and lengths of the fine-tune step, on the device: what ImageLmdb.__getitem__ does per sample
    in a dataloader worker (dataset/dataset_lmdb.py:181-204), for a whole batch in one launch.  Owns the vocabulary of `voc_type`
    (`classes`, `class_to_idx`, `idx_to_class`, :70-72).  `LOWERCASE` folds on the host -- `str.lower()` can change a word's length -- the
    rest (class lookup, UNKNOWN for anything else, EOS, PADDING, length) happens in `dig_encode_labels`."""

    def __init__(self, voc_type="ALLCASES_SYMBOLS", max_len=25, device="cuda"):
        if voc_type not in VOC_TYPES:
            raise ValueError(f"voc_type must be one of {VOC_TYPES}, not {voc_type!r}")
        if max_len < 1:
            raise ValueError("max_len must be at least 1")
        self.voc_type, self.max_len, self.device = voc_type, int(max_len), torch.device(device)
        self.classes = find_classes(voc_type)
        self.class_to_idx = dict(zip(self.classes, range(len(self.classes))))
        self.idx_to_class = dict(zip(range(len(self.classes)), self.classes))
        self.use_lowercase = voc_type == "LOWERCASE"
        self.eos, self.padding, self.unknown = (self.class_to_idx[k] for k in ("EOS", "PADDING", "UNKNOWN"))
        self.class_of_host = torch.tensor([self.class_to_idx.get(chr(c), -1) for c in range(128)], dtype=torch.int32)
        self._class_of = None

    @property
    def nb_classes(self):
        return len(self.classes)

    def class_of(self):
        if self._class_of is None:
            self._class_of = self.class_of_host.to(self.device)
        return self._class_of

    def normalize(self, word):
        """The word as the datasets label it (dataset_lmdb.py:182-183)."""
        return word.lower() if self.use_lowercase else word

    def __call__(self, words):
        words = [self.normalize(w) for w in words]
        for w in words:
            if len(w) + 1 > self.max_len:
                raise ValueError(f"word {w!r} has {len(w)} characters: with EOS it does not fit max_len = {self.max_len}")
        return encode_code_points([[ord(c) for c in w] for w in words], self.class_of(), self.eos, self.padding, self.unknown, self.max_len,
                                  self.device)
