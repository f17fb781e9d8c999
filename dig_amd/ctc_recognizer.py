"""`CTCRecModel` on the MI355X -- SURVEY.md 8(f) row N1, the third recognition head (`--decoder_type ctc`): the fine-tune encoder, the
mean over the 8 rows of the token grid, and a per-column classifier over nb_classes + 1 symbols (the last one the CTC blank).

Mirrored from the reference: the model (models/model_builder.py:8-38: `encoder`, then `ctc_classifier` = Linear(D, 512), LayerNorm(512,
eps 1e-6), GELU, Linear(512, nb_classes + 1) on `enc_x.view(B, 8, 32, D).mean(1)`; state-dict keys `encoder.*`,
`ctc_classifier.{0,1,3}.{weight,bias}`; PyTorch's default initialisation; `no_weight_decay` / `get_num_layers`) and the string rule
(`ctc_get_str_list`, evaluation_metric/metrics.py:205-244, blank = len(classes)).  The reference's `main` raises for this model and has no
criterion for it, so these are this project's own definitions: the criterion is the standard CTC loss summed over the samples and divided
by B (the `sample_normalize` convention of SeqCrossEntropyLoss), with `zero_infinity`; the labels of a target row are its cells in front of
EOS (`len_offset` = 1 on the datasets' lengths, which count EOS); `decode` returns decoder-shaped rows (emitted classes, EOS, PADDING) with the
emitting frames' softmax probabilities as scores.  `--ctc_beam_width K` (own flag, 1..32; `ctc_beam_width` here) makes the evaluation decode a
prefix beam search of width K, which scores a string by the sum over all its alignments where greedy decoding scores the single best
alignment; the rule is this project's (the reference has no CTC beam search) and stands in include/dig_hip.h at `dig_ctc_beam_decode`; its
rows carry the string's probability in score[:, 0] and 1 elsewhere.  `--ctc_lexicon FILE` (own flag; `ctc_lexicon` here, a `LabelLexicon`)
makes the evaluation decode the lexicon word of highest likelihood: `dig_ctc_lexicon_decode` scores every (image, word) pair by the sum over
all alignments, the quantity the criterion computes, where the reference's lexicon metrics snap a decoded string to the nearest word by edit
distance; rows as the beam's.  Training-mode decodes (the loop's class accuracy) stay greedy.  `align` (own; `--ctc_align_out FILE`) answers
where in the crop each character of a string is and how sure the model is of it: `dig_ctc_align` finds the best single alignment of given
labels -- a target row, or the row of any of the three decoders -- and returns every label's frames and its log-probability over them (the
rule: include/dig_hip.h; `evaluation_metric.CTCAlignment` turns them into character boxes, `frame_columns` crop columns per frame).

Flat arenas, one autograd node, the encoder on the pre-training hot-path kernels (model and step on dig_amd.finetune.EncoderTrain / _EncoderStep); the head is
`dig_window_pool_*` (the `--use_1d_attdec` pooling), two GEMMs and the fused LayerNorm + GELU launch; loss, gradient and decode are
csrc/ctc.hip.  There is no CPU fallback."""
import numpy as np
import torch

from . import _lib as L
from . import ops
from .finetune import EncoderTrain, _EncoderStep, CLS_PAD

BF16, F32 = torch.bfloat16, torch.float32
PRE = "ctc_classifier."
D_EMBEDDING = 512                                       # model_builder.py:13


# ---------------------------------------------------------------------------------------------- the entry points
def ctc_loss(logits, C, target, length, blank, len_offset=1):
    """dig_ctc_loss on logits fp32 [B, T, ld >= C]: (nll [B], loss [1])."""
    B, T, ld = logits.shape
    nll = torch.empty(B, device=logits.device, dtype=F32)
    loss = torch.empty(1, device=logits.device, dtype=F32)
    L.call("dig_ctc_loss", L.ptr(logits), ld, L.ptr(target), target.shape[1], L.ptr(length), len_offset, B, T, C, blank, L.ptr(nll), L.ptr(loss),
           L.stream())
    return nll, loss


def ctc_loss_bwd(logits, C, target, length, blank, len_offset=1, gscalar=None, ldd=None, f32=False, out=None):
    """dig_ctc_loss_bwd: d loss / d logits * gscalar as [B, T, ldd] rows (bf16, or fp32 with f32), pad columns zero."""
    B, T, ld = logits.shape
    ldd = C if ldd is None else ldd
    dl = torch.empty((B, T, ldd), device=logits.device, dtype=F32 if f32 else BF16) if out is None else out
    L.call("dig_ctc_loss_bwd", L.ptr(logits), ld, L.ptr(target), target.shape[1], L.ptr(length), len_offset, L.ptr(gscalar), B, T, C, blank,
           L.ptr(dl), ldd, int(dl.dtype == F32), L.stream())
    return dl


def ctc_greedy_decode(logits, C, blank, eos, padding):
    """dig_ctc_greedy_decode on logits fp32 [B, T, ld >= C]: (ids int64 [B, T + 1], score fp32 [B, T + 1], n int32 [B])."""
    B, T, ld = logits.shape
    dev = logits.device
    ids = torch.empty((B, T + 1), device=dev, dtype=torch.int64)
    score = torch.empty((B, T + 1), device=dev, dtype=F32)
    n = torch.empty(B, device=dev, dtype=torch.int32)
    L.call("dig_ctc_greedy_decode", L.ptr(logits), ld, B, T, C, blank, eos, padding, L.ptr(ids), L.ptr(score), L.ptr(n), L.stream())
    return ids, score, n


MAX_BEAM_WIDTH = 32                                     # csrc/ctc.hip: one lane per hypothesis, the candidate table in LDS


def ctc_beam_decode(logits, C, blank, eos, padding, beam_width):
    """dig_ctc_beam_decode (prefix beam search, the rule in include/dig_hip.h) on logits fp32 [B, T, ld >= C]: (ids int64 [B, T + 1],
    score fp32 [B, T + 1] = exp(logp) then 1, logp fp32 [B], n int32 [B])."""
    B, T, ld = logits.shape
    dev = logits.device
    ids = torch.empty((B, T + 1), device=dev, dtype=torch.int64)
    score = torch.empty((B, T + 1), device=dev, dtype=F32)
    logp = torch.empty(B, device=dev, dtype=F32)
    n = torch.empty(B, device=dev, dtype=torch.int32)
    L.call("dig_ctc_beam_decode", L.ptr(logits), ld, B, T, C, blank, eos, padding, int(beam_width), L.ptr(ids), L.ptr(score), L.ptr(logp), L.ptr(n),
           L.stream())
    return ids, score, logp, n


def ctc_align(logits, C, target, length, blank, len_offset=1, want_frames=False):
    """dig_ctc_align (forced alignment, the rule in include/dig_hip.h) on logits fp32 [B, T, ld >= C]: the best path of the labels of
    target int64 [B, ldt] (row b: its first length[b] - len_offset cells) through the frames.  Returns (start int32 [B, ldt], end int32
    [B, ldt]: label k on frames [start, end), -1 past the labels; char_logp fp32 [B, ldt]: the label's log-probability summed over its
    frames; path_logp fp32 [B]: the whole path's, -inf for a sample without an alignment) and, with want_frames, frame_label int32 [B, T]
    (the label index of every frame, -1 on a blank frame, -2 without an alignment)."""
    B, T, ld = logits.shape
    dev, ldt = logits.device, target.shape[1]
    start = torch.empty((B, ldt), device=dev, dtype=torch.int32)
    end = torch.empty((B, ldt), device=dev, dtype=torch.int32)
    char_logp = torch.empty((B, ldt), device=dev, dtype=F32)
    path_logp = torch.empty(B, device=dev, dtype=F32)
    frames = torch.empty((B, T), device=dev, dtype=torch.int32) if want_frames else None
    L.call("dig_ctc_align", L.ptr(logits), ld, L.ptr(target), ldt, L.ptr(length), len_offset, B, T, C, blank, L.ptr(start), L.ptr(end),
           L.ptr(char_logp), L.ptr(path_logp), L.ptr(frames), L.stream())
    return (start, end, char_logp, path_logp, frames) if want_frames else (start, end, char_logp, path_logp)


LEX_CHUNK = L.const("DIG_CTC_LEX_CHUNK")                # words per workgroup of the lexicon decode
MAX_LEX_WORD_LEN = 63                                   # csrc/ctc.hip: lane i of a wave owns label i, lane n the final blank


def ctc_lexicon_workspace_bytes(B, T, C, max_count):
    return L.query("dig_ctc_lexicon_workspace_bytes", B, T, C, max_count)


def ctc_lexicon_decode(logits, C, blank, eos, padding, pool, lex_begin, lex_count, want_scores=False):
    """dig_ctc_lexicon_decode (the rule in include/dig_hip.h) on logits fp32 [B, T, ld >= C]: sample b takes the word of highest CTC
    likelihood among pool rows [lex_begin[b], lex_begin[b] + lex_count[b]).  pool: a `LabelLexicon`, or (labels int32 [W, ldw], lengths
    int32 [W]) on the logits' device.  lex_begin / lex_count are host sequences; a range outside the pool is refused here, before upload.
    Returns (best_index int32 [B] (-1: no word), logp fp32 [B], ids int64 [B, T + 1], score fp32 [B, T + 1] = exp(logp) then 1, n int32 [B])
    and, with want_scores, scores fp32 [B, max(lex_count)] (log-likelihood per range position, -inf past the range)."""
    B, T, ld = logits.shape
    dev = logits.device
    words, word_len = pool.device(dev) if isinstance(pool, LabelLexicon) else pool
    W = pool.n_rows if isinstance(pool, LabelLexicon) else words.shape[0]
    begin, count = np.asarray(lex_begin, dtype=np.int64).reshape(-1), np.asarray(lex_count, dtype=np.int64).reshape(-1)
    if begin.shape != (B,) or count.shape != (B,):
        raise ValueError(f"lex_begin / lex_count need one entry per sample ({B})")
    bad = np.nonzero((begin < 0) | (count < 0) | (begin + count > W))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"lexicon range of sample {b} ([{int(begin[b])}, {int(begin[b] + count[b])})) is outside the pool of {W} words")
    if words.shape[0] == 0:                                                # (an empty tensor has no address to hand over)
        words, word_len = torch.zeros((1, max(words.shape[1], 1)), device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
    max_count = int(count.max()) if B else 0
    best_index = torch.empty(B, device=dev, dtype=torch.int32)
    logp = torch.empty(B, device=dev, dtype=F32)
    ids = torch.empty((B, T + 1), device=dev, dtype=torch.int64)
    score = torch.empty((B, T + 1), device=dev, dtype=F32)
    n = torch.empty(B, device=dev, dtype=torch.int32)
    scores = torch.empty((B, max_count), device=dev, dtype=F32) if want_scores else None
    if B:
        ranges = torch.from_numpy(np.stack([begin, count]).astype(np.int32)).to(dev)
        ws_bytes = ctc_lexicon_workspace_bytes(B, T, C, max_count)
        ws = torch.empty(ws_bytes // 8 + 1, device=dev, dtype=torch.int64)
        L.call("dig_ctc_lexicon_decode", L.ptr(logits), ld, B, T, C, blank, eos, padding, L.ptr(words), L.ptr(word_len), words.shape[1], W,
               L.ptr(ranges[0]), L.ptr(ranges[1]), max_count, L.ptr(best_index), L.ptr(logp), L.ptr(ids), L.ptr(score), L.ptr(n),
               L.ptr(scores) if want_scores and max_count else None, L.ptr(ws), ws_bytes, L.stream())
    return (best_index, logp, ids, score, n, scores) if want_scores else (best_index, logp, ids, score, n)


_VOC_BY_CLASSES = {71: "LOWERCASE", 65: "ALLCASES", 97: "ALLCASES_SYMBOLS"}     # len(datasets.find_classes(voc_type))


class LabelLexicon:
    """Host preparation of a lexicon for `ctc_lexicon_decode`, done once: `{name: [words]}` (per-image lexicons; identical lists are stored
    once and share their range) or one flat list of words (name None), as rows of class ids.

    A word is encoded by the datasets' `LabelEncoder` rule of `voc_type`: `normalize` applies (a LOWERCASE vocabulary folds) and a character
    outside the vocabulary becomes UNKNOWN, an ordinary class.  For the case-sensitive vocabularies (ALLCASES, ALLCASES_SYMBOLS) a word
    contributes up to four rows: as written, lower(), upper() and capitalize(), de-duplicated per word (`casings=False`: as written only),
    so that an upper-case benchmark lexicon can match a model that writes lower case.  `row_word[r]` is the index into `words` (the raw
    words of all lists, in order) of the raw word row r stands for; `word_of(r)` is that word.  A word of more than 63 labels is refused.

    Row order: within a range the rows are sorted by length, then by original order (word by word, casings in the order above).  The decode
    takes the first row among equal likelihoods, so its tie rule reads: shortest first, then first listed.  Sorting also keeps words of
    one length in one workgroup, which lets the kernel pack four short words into a wave.  `device(dev)` uploads once per device."""

    def __init__(self, words, voc_type="ALLCASES_SYMBOLS", casings=None):
        from .datasets import LabelEncoder
        enc = LabelEncoder(voc_type, MAX_LEX_WORD_LEN + 1, "cpu")          # (the vocabulary and `normalize` only: nothing is launched)
        self.voc_type, self.nb_classes = voc_type, enc.nb_classes
        self.casings = (voc_type != "LOWERCASE") if casings is None else bool(casings)
        by_name = words if isinstance(words, dict) else {None: list(words)}
        self.ranges, self._lists, self.words = {}, {}, []
        rows, row_word, seen = [], [], {}
        for name, lst in by_name.items():
            key = tuple(lst)
            r = seen.get(key)
            if r is None:
                base, mine = len(self.words), []
                for i, w in enumerate(key):
                    forms = (w, w.lower(), w.upper(), w.capitalize()) if self.casings else (w,)
                    done = set()
                    for f in forms:
                        labels = tuple(enc.class_to_idx.get(c, enc.unknown) for c in enc.normalize(f))
                        if len(labels) > MAX_LEX_WORD_LEN:
                            raise ValueError(f"lexicon word longer than {MAX_LEX_WORD_LEN} labels ({len(labels)}) in {name!r}: {w!r}")
                        if labels not in done:
                            done.add(labels)
                            mine.append((len(labels), len(mine), labels, base + i))
                mine.sort(key=lambda t: t[:2])
                r = seen[key] = (len(rows), len(mine), list(key))
                rows.extend(t[2] for t in mine)
                row_word.extend(t[3] for t in mine)
                self.words.extend(key)
            self.ranges[name] = r[:2]
            self._lists[name] = r[2]
        self.n_rows = len(rows)
        ld = max([len(r) for r in rows] + [1])
        self.labels, self.label_len = np.zeros((max(self.n_rows, 1), ld), dtype=np.int32), np.zeros(max(self.n_rows, 1), dtype=np.int32)
        for i, r in enumerate(rows):
            self.labels[i, :len(r)] = r
            self.label_len[i] = len(r)
        self.row_word = np.asarray(row_word, dtype=np.int64)
        self._dev, self._norm_host, self._norm_dev = {}, None, {}

    def __getitem__(self, name):
        return self._lists[name]

    def __contains__(self, name):
        return name in self._lists

    def __len__(self):
        return len(self._lists)

    def keys(self):
        return self._lists.keys()

    def word_of(self, row):
        """The raw word pool row `row` stands for; None for -1 (no word)."""
        return None if row < 0 else self.words[int(self.row_word[row])]

    def device(self, dev):
        """(labels int32 [max(n_rows, 1), ld], lengths int32) on `dev`."""
        dev = torch.device(dev)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = (torch.from_numpy(self.labels).to(dev), torch.from_numpy(self.label_len).to(dev))
        return t

    def normalized_words(self, dev):
        """What the lexicon metrics compare with a normalised target, on `dev` (built once, uploaded once per device): the raw words under
        evaluation_metric._normalize_text as code-point rows (int32 [max(len(words), 1), ld]) with their lengths (int32), indexed like
        `words`, and `row_word` as int32 [n_rows]."""
        from .evaluation_metric import _normalize_text, _pool
        dev = torch.device(dev)
        t = self._norm_dev.get(dev)
        if t is None:
            if self._norm_host is None:
                self._norm_host = _pool([_normalize_text(w) for w in self.words]) + (self.row_word.astype(np.int32),)
            t = self._norm_dev[dev] = tuple(torch.from_numpy(a).to(dev) for a in self._norm_host)
        return t


def read_lexicon_file(path):
    """The words of a UTF-8 file with one word per line; empty lines are skipped."""
    with open(path, encoding="utf-8") as f:
        return [w for w in (line.strip() for line in f) if w]


def match_widths(pred, target, padding):
    """Two [B, *] label tensors at one width (what dig_string_match and its kin compare): the narrower one padded with PADDING."""
    target = target.to(pred.device).long()
    wp, wt = pred.shape[1], target.shape[1]
    if wp == wt:
        return pred, target
    wide = torch.full((pred.shape[0], max(wp, wt)), padding, device=pred.device, dtype=torch.int64)
    if wp < wt:
        wide[:, :wp] = pred
        return wide, target
    wide[:, :wt] = target
    return pred, wide


class _SeqCTCFn(torch.autograd.Function):
    """The CTC launch and its gradient (fp32 rows, as wide as the logits)."""

    @staticmethod
    def forward(ctx, logits, target, length, blank, len_offset):
        x = logits.detach().float().contiguous()
        _, loss = ctc_loss(x, x.shape[2], target, length, blank, len_offset)
        ctx.save_for_backward(x, target, length)
        ctx.cfg = (blank, len_offset)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, target, length = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()                         # (named: a converted copy must outlive the call)
        blank, len_offset = ctx.cfg
        return ctc_loss_bwd(x, x.shape[2], target, length, blank, len_offset, gscalar=gs, f32=True), None, None, None, None


class SeqCTCLoss(torch.nn.Module):
    """The criterion of the CTC head: forward(logits [B, T, nb_classes + 1] fp32, target [B, max_len], length [B]) -> 0-dim loss =
    sum_b -log p(labels_b | logits_b) / B with zero_infinity; the labels of row b are its first length[b] - len_offset cells (the datasets'
    lengths count the closing EOS: len_offset = 1).  `blank` None: the last class of the logits."""

    def __init__(self, blank=None, len_offset=1):
        super().__init__()
        self.blank, self.len_offset = blank, int(len_offset)

    def forward(self, input, target, length):
        blank = input.shape[-1] - 1 if self.blank is None else int(self.blank)
        return _SeqCTCFn.apply(input, target.to(input.device).long().contiguous(), length.to(input.device).long().contiguous(), blank, self.len_offset)

    def extra_repr(self):
        return f"blank={self.blank}, len_offset={self.len_offset}"


# ---------------------------------------------------------------------------------------------- the model
class _CTCTrainStep(_EncoderStep):
    """Forward / backward of one CTCRecModel step."""

    def head_forward(self, enc):
        """ctc_classifier on the column means of the token grid: enc bf16 [B*256, D] -> logits fp32 [B*32, CLS_PAD] (columns past
        nb_classes + 1: zero weights) and what the backward reads."""
        M, p, w = self.m, self.p, self.w
        B = enc.shape[0] // M.N
        rows = B * M.gw
        cols = torch.empty((rows, M.D), device=enc.device, dtype=BF16)
        ops.window_pool_fwd(enc, cols, B, M.gh, M.gw, M.gw, M.D)
        h = ops.linear_fwd(cols, w(PRE + "0.weight"), bias=p(PRE + "0.bias"))
        a, mu, rs = ops.layernorm_fwd(h, p(PRE + "1.weight"), p(PRE + "1.bias"), 1e-6, gelu=True)
        self.cls_w, cb = M.padded_classifier(PRE + "3.weight", PRE + "3.bias", CLS_PAD)
        logits = torch.empty((rows, CLS_PAD), device=enc.device, dtype=F32)
        ops.gemm(a, self.cls_w, rows, CLS_PAD, D_EMBEDDING, out=logits, out_kind=ops.OUT_F32, bias=cb)
        return logits, (cols, h, mu, rs, a)

    def forward(self, images, targets, lens):
        M = self.m
        enc = self.encoder_forward(images)
        logits, self.saved = self.head_forward(enc)
        C1 = M.nb_classes + 1
        return logits[:, :C1].reshape(self.B, M.gw, C1)

    def backward(self, dlogits_btc):
        M = self.m
        dev = dlogits_btc.device
        main, sd = self.begin_backward(dev)
        side, p, w, g = self.side, self.p, self.w, self.g
        B, C1 = self.B, M.nb_classes + 1
        rows = B * M.gw
        cols, h, mu, rs, a = self.saved
        dl = torch.zeros((rows, CLS_PAD), device=dev, dtype=BF16)
        dl[:, :C1] = dlogits_btc.reshape(rows, C1).to(BF16)
        da = self.classifier_backward(dl, a, PRE + "3.weight", PRE + "3.bias", classes=C1)
        dh = ops.layernorm_bwd(da, h, p(PRE + "1.weight"), p(PRE + "1.bias"), mu, rs, None, g(PRE + "1.weight"), g(PRE + "1.bias"), gelu=True)
        side(lambda: ops.linear_wgrad(dh, cols, g(PRE + "0.weight")), dh, cols)
        side(lambda: ops.colsum(dh, g(PRE + "0.bias")), dh)
        dcols = ops.linear_dgrad(dh, w(PRE + "0.weight"))
        denc = torch.empty((B * M.N, M.D), device=dev, dtype=BF16)          # every token of a column gets 1/gh of the column's gradient
        ops.window_pool_bwd(dcols, denc, B, M.gh, M.gw, M.gw, M.D, False)
        self.encoder_backward(denc)
        main.wait_stream(sd)


class CTCRecModelTrain(EncoderTrain):
    """models.model_builder.CTCRecModel: `.train()` forward = (logits [B, 32, nb_classes + 1] fp32, None, None, None) with autograd,
    `.eval()` forward = the same logits from the walk without dropout; `decode(logits)` = the CTC strings as decoder-shaped rows, greedy or,
    with `ctc_beam_width` K > 0 (args.ctc_beam_width) in eval mode, by prefix beam search of width K, or, with `ctc_lexicon` set (a
    `LabelLexicon` over one flat list; args.ctc_lexicon: such an object, a list of words or a word file), in eval mode the lexicon word
    of highest likelihood for every sample."""
    _step_cls = _CTCTrainStep
    is_ctc = True
    _LAYER_NORMS = (PRE + "1.",)                        # (the head keeps PyTorch's defaults: CTCRecModel applies no init of its own)

    def __init__(self, args=None, *, ctc_beam_width=None, ctc_lexicon=None, **kw):
        if ctc_beam_width is None:
            ctc_beam_width = getattr(args, "ctc_beam_width", 0) or 0
        if not 0 <= int(ctc_beam_width) <= MAX_BEAM_WIDTH:
            raise ValueError(f"ctc_beam_width {ctc_beam_width}: 0 (greedy) or a prefix beam search of width 1..{MAX_BEAM_WIDTH}")
        if ctc_lexicon is None:
            ctc_lexicon = getattr(args, "ctc_lexicon", None) or None
        if ctc_lexicon is not None and int(ctc_beam_width) > 0:
            raise ValueError("ctc_lexicon with ctc_beam_width > 0: an evaluation decodes by one rule")
        super().__init__(args, **kw)
        nb_classes = self.nb_classes
        if nb_classes + 1 > CLS_PAD:
            raise NotImplementedError(f"nb_classes + 1 above {CLS_PAD}: the classifier is padded to {CLS_PAD} rows")
        if nb_classes < 3:
            raise ValueError("nb_classes counts EOS, PADDING and UNKNOWN, the last three classes of a vocabulary")
        self.blank = nb_classes                                             # blank_label = len(classes) (metrics.py:211)
        self.eos, self.padding = nb_classes - 3, nb_classes - 2             # a vocabulary ends in EOS, PADDING, UNKNOWN (datasets.find_classes)
        self.ctc_beam_width = int(ctc_beam_width)                           # what `decode` runs in eval mode: 0 = greedy
        if ctc_lexicon is not None and not isinstance(ctc_lexicon, LabelLexicon):
            voc_type = getattr(args, "voc_type", None) or _VOC_BY_CLASSES.get(nb_classes)
            if voc_type is None:
                raise ValueError(f"ctc_lexicon: no vocabulary type has {nb_classes} classes; pass a LabelLexicon")
            ctc_lexicon = LabelLexicon(read_lexicon_file(ctc_lexicon) if isinstance(ctc_lexicon, str) else list(ctc_lexicon), voc_type)
        if ctc_lexicon is not None:
            if None not in ctc_lexicon or len(ctc_lexicon) != 1:
                raise ValueError("ctc_lexicon: a LabelLexicon over one flat list of words")
            if ctc_lexicon.nb_classes != nb_classes:
                raise ValueError(f"ctc_lexicon is encoded for {ctc_lexicon.nb_classes} classes ({ctc_lexicon.voc_type}), the model has {nb_classes}")
        self.ctc_lexicon = ctc_lexicon                                      # eval-mode `decode`: the most probable word of this list

    def head_shapes(self):
        o = {PRE + "0.weight": (D_EMBEDDING, self.D), PRE + "0.bias": (D_EMBEDDING,), PRE + "1.weight": (D_EMBEDDING,), PRE + "1.bias": (D_EMBEDDING,)}
        o[PRE + "3.weight"] = (self.nb_classes + 1, D_EMBEDDING); o[PRE + "3.bias"] = (self.nb_classes + 1,)
        return o

    @torch.no_grad()
    def logits(self, images):
        """The eval forward: the training step's walk without dropout keys (and, like it, with the blocks' activations kept)."""
        step, enc = self.eval_tokens(images)
        C1 = self.nb_classes + 1
        return step.head_forward(enc)[0][:, :C1].reshape(images.shape[0], self.gw, C1)

    def decode(self, logits, beam_width=None):
        """(ids int64 [B, 33], score fp32 [B, 33], n int32 [B]) of logits [B, 32, nb_classes + 1].  beam_width 0: csrc/ctc.hip's greedy
        rule (scores: the emitting frames' probabilities); K > 0: its prefix beam search of width K (score[:, 0]: the probability of the
        string over all its alignments).  None: `ctc_beam_width` in eval mode and 0 while training (the class accuracy of the training loop
        stays the greedy one).  With `ctc_lexicon` set, beam_width None in eval mode is csrc/ctc.hip's lexicon decode: every sample gets
        the word of the list with the highest likelihood (rows as the beam's; the empty row when no word can be aligned)."""
        x = logits.detach().float().contiguous()
        lex = getattr(self, "ctc_lexicon", None)
        if beam_width is None and not self.training and lex is not None:
            begin, count = lex.ranges[None]
            _, _, ids, score, n = ctc_lexicon_decode(x, x.shape[2], self.blank, self.eos, self.padding, lex, [begin] * x.shape[0], [count] * x.shape[0])
            return ids, score, n
        if beam_width is None:
            beam_width = 0 if self.training else self.ctc_beam_width
        if beam_width == 0:
            return ctc_greedy_decode(x, x.shape[2], self.blank, self.eos, self.padding)
        ids, score, _, n = ctc_beam_decode(x, x.shape[2], self.blank, self.eos, self.padding, beam_width)
        return ids, score, n

    frame_columns = 128 // EncoderTrain.gw               # crop columns per frame: the head classifies the 32 column means of a patch-4 grid

    def align(self, logits, rows, lengths, len_offset=1):
        """(start, end, char_logp, path_logp) of csrc/ctc.hip's forced alignment of `rows` through logits [B, 32, nb_classes + 1]: dataset
        targets with their lengths (which count the closing EOS: len_offset = 1), or, with len_offset = 0, the (ids, n) that `decode`
        returned, whichever decoder produced them.  Character k of row b covers the crop columns [start * frame_columns, end *
        frame_columns).  Cells past a row's labels hold -1 / 0; a row wider than 63 cells is cut to 63."""
        x = logits.detach().float().contiguous()
        rows = rows.to(x.device).long()[:, :MAX_LEX_WORD_LEN].contiguous()
        return ctc_align(x, x.shape[2], rows, lengths.to(x.device).long().contiguous(), self.blank, len_offset)

    def forward(self, x):
        if self.training:
            return super().forward(x)
        return self.logits(self._device_images(x)), None, None, None
