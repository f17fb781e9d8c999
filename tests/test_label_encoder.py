"""dig_encode_labels (csrc/labels.hip, cpu_abi/dig_cpu_rec.cpp) and its host wrapper dig_amd.datasets.LabelEncoder: words -> the target rows
and lengths of the fine-tune step.  Integer work: every comparison is exact, on both builds of the ABI."""
import ctypes
import string

import numpy as np
import pytest
import torch

VOC_TYPES = ("LOWERCASE", "ALLCASES", "ALLCASES_SYMBOLS")


# ---------------------------------------------------------------------------------------------- the reference, restated
def ref_classes(voc_type):
    """dataset/dataset_lmdb.py:75-97."""
    if voc_type == "LOWERCASE":
        voc = list('0123456789abcdefghijklmnopqrstuvwxyz!"#$%&\'()*+,-./:;<=>?@[\\]^_`{|}~')
    elif voc_type == "ALLCASES":
        voc = list(string.digits + string.ascii_letters)
    else:
        voc = list(string.printable[:-6])
    return voc + ["EOS", "PADDING", "UNKNOWN"]


def ref_encode(word, class_to_idx, max_len):
    """dataset/dataset_lmdb.py:189-204, line for line (`word` as it stands there: already lower-cased under LOWERCASE)."""
    label = np.full((max_len,), class_to_idx['PADDING'], dtype=np.int64)
    label_list = []
    for char in word:
        if char in class_to_idx:
            label_list.append(class_to_idx[char])
        else:
            label_list.append(class_to_idx['UNKNOWN'])
    label_list = label_list + [class_to_idx['EOS']]
    assert len(label_list) <= max_len
    label[:len(label_list)] = np.array(label_list)
    label_len = len(label_list)
    return label, label_len


def ref_batch(words, voc_type, max_len):
    c2i = {c: i for i, c in enumerate(ref_classes(voc_type))}
    rows = [ref_encode(w, c2i, max_len) for w in words]
    return torch.from_numpy(np.stack([r[0] for r in rows])), torch.tensor([r[1] for r in rows], dtype=torch.int64)


def word_set(voc_type, max_len, n):
    """n words: the edge cases first, seeded random words of every length 0 .. max_len - 1 behind them."""
    rng = np.random.RandomState(max_len * 7 + len(voc_type))
    chars = ref_classes(voc_type)[:-3]
    edge = ["",                                                       # [EOS, PADDING, ...], lens 1
            "".join(chars[i % len(chars)] for i in range(max_len - 2)),   # the longest word the datasets let through
            "".join(chars[(3 * i) % len(chars)] for i in range(max_len - 1)),   # just fits: EOS in the last cell, no padding
            "Hello World",                                            # a space (no vocabulary has one); upper case
            "a b!", "~", "\x7f\x80",                                 # 127 and 128
            "x中y", "\U0001F600", "ok\U0001F600中\x7f",       # beyond ASCII: one label per code point
            "\x00\x1f"]
    words = list(edge[:n])
    while len(words) < n:
        k = rng.randint(0, max_len)
        pool = chars + [" ", "é", "A", "z"]
        words.append("".join(pool[i] for i in rng.randint(0, len(pool), size=k)))
    return words


def fold(words, voc_type):
    return [w.lower() for w in words] if voc_type == "LOWERCASE" else list(words)


# ---------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("max_len", [25, 100])
@pytest.mark.parametrize("voc_type", VOC_TYPES)
def test_encoder_equals_the_reference_rule(abi_dev, voc_type, max_len):
    from dig_amd.datasets import LabelEncoder
    enc = LabelEncoder(voc_type, max_len, abi_dev)
    assert enc.classes == ref_classes(voc_type)
    assert enc.class_to_idx == {c: i for i, c in enumerate(enc.classes)} and enc.idx_to_class == dict(enumerate(enc.classes))
    for B in (1, 63, 65, 257):                                        # the last wave of the launch is partial for each of them
        words = [w for w in fold(word_set(voc_type, max_len, B), voc_type) if len(w) + 1 <= max_len][:B]
        while len(words) < B:                                         # (lower-casing can lengthen a word past the row)
            words.append("pad")
        assert len(words) == B
        labels, lens = enc(words)
        want, want_lens = ref_batch(words, voc_type, max_len)
        assert labels.dtype == torch.int64 and lens.dtype == torch.int64 and tuple(labels.shape) == (B, max_len)
        assert torch.equal(labels.cpu(), want), [w for w, g, r in zip(words, labels.cpu(), want) if not torch.equal(g, r)][:3]
        assert torch.equal(lens.cpu(), want_lens)


@pytest.mark.parametrize("max_len", [25, 100])
def test_edge_rows(abi_dev, max_len):
    from dig_amd.datasets import LabelEncoder
    enc = LabelEncoder("ALLCASES_SYMBOLS", max_len, abi_dev)
    assert enc.nb_classes == 97 and enc.eos == 94 and enc.padding == 95 and enc.unknown == 96    # what the decode kernels assume
    labels, lens = enc([""])                                          # B = 1, the empty word
    assert labels.cpu().tolist() == [[94] + [95] * (max_len - 1)] and lens.cpu().tolist() == [1]
    full = "q" * (max_len - 1)                                        # just fits
    labels, lens = enc([full, "q" * (max_len - 2)])
    row = labels.cpu()
    assert row[0, -1] == 94 and (row[0] != 95).all() and lens.cpu().tolist() == [max_len, max_len - 1]
    assert row[1, -2] == 94 and row[1, -1] == 95
    labels, lens = enc(["\x7f\x80中\U0001F600 a"])               # 127, 128, a CJK character, an emoji, a space: UNKNOWN, one label each
    assert labels.cpu()[0, :7].tolist() == [96, 96, 96, 96, 96, enc.class_to_idx["a"], 94] and lens.item() == 7
    labels, lens = enc([])                                            # B = 0: no launch, empty results
    assert tuple(labels.shape) == (0, max_len) and tuple(lens.shape) == (0,)


@pytest.mark.parametrize("max_len", [25, 100])
def test_characters_outside_the_vocabulary(abi_dev, max_len):
    """An upper-case letter under LOWERCASE reached without the host's folding, a space under ALLCASES: UNKNOWN."""
    from dig_amd.datasets import LabelEncoder, encode_code_points
    low = LabelEncoder("LOWERCASE", max_len, abi_dev)
    labels, lens = encode_code_points([[ord(c) for c in "aBc"]], low.class_of(), low.eos, low.padding, low.unknown, max_len, abi_dev)
    want, want_lens = ref_batch(["aBc"], "LOWERCASE", max_len)        # (the reference's loop on the unfolded word)
    assert torch.equal(labels.cpu(), want) and labels.cpu()[0, 1] == low.unknown and torch.equal(lens.cpu(), want_lens)
    assert torch.equal(low(["aBc"])[0].cpu(), ref_batch(["abc"], "LOWERCASE", max_len)[0])       # folded by the wrapper
    allc = LabelEncoder("ALLCASES", max_len, abi_dev)
    labels, _ = allc(["A b"])
    assert labels.cpu()[0, :4].tolist() == [allc.class_to_idx["A"], allc.unknown, allc.class_to_idx["b"], allc.eos]


# ---------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("max_len", [25, 100])
@pytest.mark.parametrize("voc_type", VOC_TYPES)
def test_round_trip_through_tokens_to_text(abi_dev, voc_type, max_len):
    from dig_amd import evaluation_metric as EM
    from dig_amd.datasets import LabelEncoder
    enc = LabelEncoder(voc_type, max_len, abi_dev)
    words = [w for w in word_set(voc_type, max_len, 65) if len(w.lower()) + 1 <= max_len]
    labels, _ = enc(words)
    text, length = EM.tokens_to_text(labels, enc.classes)
    text, length = text.cpu(), length.cpu()
    for i, w in enumerate(words):
        want = [ord(c) for c in EM._normalize_text(w)]                # (every vocabulary holds 0-9 and a-z; A-Z is held or folded)
        assert text[i, :int(length[i])].tolist() == want, w


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("max_len", [25, 100])
def test_refusals_before_any_launch(abi_dev, max_len):
    from dig_amd import _lib as L
    from dig_amd.datasets import LabelEncoder
    enc = LabelEncoder("ALLCASES_SYMBOLS", max_len, abi_dev)
    with pytest.raises(ValueError, match="x" * max_len):
        enc(["ok", "x" * max_len])                                    # max_len characters: no room for EOS
    enc(["x" * (max_len - 1)])
    f = L.lib().dig_encode_labels
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    chars = torch.zeros(4, dtype=torch.int32, device=abi_dev)
    offs = torch.tensor([0, 2, 4], dtype=torch.int32, device=abi_dev)
    labels = torch.full((2, max_len), -7, dtype=torch.int64, device=abi_dev)
    lens = torch.full((2,), -7, dtype=torch.int64, device=abi_dev)
    ok = [L.ptr(chars), L.ptr(offs), L.ptr(enc.class_of()), 94, 95, 96, max_len, 2, L.ptr(labels), L.ptr(lens), L.stream()]
    bad = L.const("DIG_ERR_ARG")
    for i in (0, 1, 2, 8, 9):                                         # every pointer
        args = list(ok)
        args[i] = None
        assert f(*args) == bad
    for i, v in ((6, 0), (6, -1), (7, -1)):                           # max_len < 1, B < 0
        args = list(ok)
        args[i] = v
        assert f(*args) == bad
    args = list(ok)
    args[7] = 0                                                       # B == 0 succeeds, nothing is written
    assert f(*args) == 0
    assert (labels.cpu() == -7).all() and (lens.cpu() == -7).all()
    assert f(*ok) == 0
    assert lens.cpu().tolist() == [3, 3]


# ---------------------------------------------------------------------------------------------- the two builds against each other
@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [25, 100])
def test_both_builds_agree_bit_for_bit(max_len):
    from cpu_abi_util import cpu_abi_backend
    from dig_amd.datasets import LabelEncoder
    got = {}
    for voc_type in VOC_TYPES:
        words = [w for w in fold(word_set(voc_type, max_len, 257), voc_type) if len(w) + 1 <= max_len]
        got[voc_type] = [t.cpu() for t in LabelEncoder(voc_type, max_len, "cuda:0")(words)]
    with cpu_abi_backend() as dev:
        for voc_type in VOC_TYPES:
            words = [w for w in fold(word_set(voc_type, max_len, 257), voc_type) if len(w) + 1 <= max_len]
            labels, lens = LabelEncoder(voc_type, max_len, dev)(words)
            assert torch.equal(labels, got[voc_type][0]) and torch.equal(lens, got[voc_type][1])
