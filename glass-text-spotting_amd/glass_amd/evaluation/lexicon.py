"""Lexicons for lexicon-constrained text evaluation (reference glass/evaluation/lexicon_utils.py).

  * `load_lexicon` - `get_lexicon` (:51-131): the MaskTextSpotterV3 lexicon files, with `root` standing in for the
    directory the reference hard-codes; returns (lexicon, pairs) in the shapes `TextResultWriter` takes.
  * `DeviceLexicon` - a word list, or a dict of per-image word lists (one segment each), upper-cased and encoded once
    and kept on the device.
  * `LexiconMatcher` - `find_match_word` (:4-28, the un-weighted branch) for a whole batch of recognised words in one
    launch of glass_lexicon_match (csrc/lexicon.hip); `TextResultWriter(matcher=...)` uses it.
  * `WeightedLexiconMatcher` - the weighted branch (:26-48 with `weighted_edit_distance`, :136-182; the evaluator's
    TEST.LEXICON_WEIGHTED) through glass_lexicon_match_weighted (csrc/lexicon_weighted.hip): the host turns each record's
    character probabilities into float64 cost tables (`weighted_cost_tables`), the device finds the candidates and runs
    the DP; `TextResultWriter(matcher=..., weighted_ed=True)` uses it.
  * `LexiconTrie` - the same lexicons as a trie over the decoder's classes, for the OTHER lexicon protocol: decoding that can
    only emit lexicon words (glass_beam_search_lexicon, `ASTER_V2.beam_decode(lexicon=...)`,
    `RecognizerRCNNHeadV3.set_lexicon`), where the matchers above repair a word after it was decoded.
    evaluation/pattern.py generalises it: `DecodePattern` is any finite automaton over the same fold symbols (a regex, a
    character set, or this trie through `DecodePattern.from_trie`).

Symbols: both sides are upper-cased with `str.upper()` as the reference does (once, at load, for the lexicon: it can
change a word's length, e.g. 'ß' -> 'SS').  Queries are ASCII (the writer strips other characters first, `de_ascii`);
every lexicon code point >= 128 becomes one sentinel byte that no query byte equals, which gives exactly the edit
distance over code points, because only query-to-word equality enters it.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

SENTINEL = 0x80               # every non-ASCII lexicon code point
MAX_QUERY = 64                # symbols of one query (one 64-bit pattern word on the device)
NO_MATCH = ("", 100)          # find_match_word's answer when no word is closer than its dist_min start value
NO_CLASS = 0xFF               # symbol -> class table entry of a symbol the text encoder has no class for
WEIGHTED_TABLE_CAP_BYTES = 256 << 20      # most bytes of cost tables uploaded for one launch (RRCScorer's workspace cap)

_LEXICON_DIR = os.path.join("evaluation", "lexicons")
_FILES = {("totaltext", "weak"): ("totaltext/weak_voc_new.txt", "totaltext/weak_voc_pair_list.txt"),
          ("icdar15", 1): ("ic15/GenericVocabulary_new.txt", "ic15/GenericVocabulary_pair_list.txt"),
          ("icdar15", 2): ("ic15/ch4_test_vocabulary_new.txt", "ic15/ch4_test_vocabulary_pair_list.txt")}
_IC15_STRONG = ("ic15/new_strong_lexicon/new_voc_img_{}.txt", "ic15/new_strong_lexicon/pair_voc_img_{}.txt")
_IC15_TEST_IMAGES = 500


def _read_words(path: str) -> List[str]:
    with open(path, "r", encoding="utf-8") as f:
        return [line.strip() for line in f.readlines()]


def _read_pairs(path: str) -> Dict[str, str]:
    """lexicon_utils.py:60-65: the key is the first space-separated field upper-cased, the value is the line from
    len(key) + 1 on (measured on the UPPER-cased key, as the reference does)."""
    pairs = {}
    with open(path, "r", encoding="utf-8") as f:
        for line in f.readlines():
            line = line.strip()
            word = line.split(" ")[0].upper()
            pairs[word] = line[len(word) + 1:]
    return pairs


def load_lexicon(root: str, dataset: str = "totaltext", lexicon_type: int = 2):
    """`get_lexicon(dataset, lexicon_type)` over `<root>/evaluation/lexicons/...` (root = a MaskTextSpotterV3 checkout).
    Type 0 -> (None, None); 'totaltext' -> the weak lexicon for ANY other type; 'icdar15' 1 -> generic, 2 -> the
    ch4_test_vocabulary (weak), 3 -> the per-image strong lexicons as dicts keyed by image id 1..500; anything else
    raises ValueError (lexicon_utils.py:131)."""
    if lexicon_type == 0:
        return None, None
    base = os.path.join(root, _LEXICON_DIR)
    if dataset == "totaltext":
        lex, pair = _FILES[("totaltext", "weak")]
        return _read_words(os.path.join(base, lex)), _read_pairs(os.path.join(base, pair))
    if dataset == "icdar15":
        if lexicon_type in (1, 2):
            lex, pair = _FILES[("icdar15", lexicon_type)]
            return _read_words(os.path.join(base, lex)), _read_pairs(os.path.join(base, pair))
        if lexicon_type == 3:
            lexicons, pairs = {}, {}
            for i in range(1, _IC15_TEST_IMAGES + 1):
                lexicons[i] = _read_words(os.path.join(base, _IC15_STRONG[0].format(i)))
                pairs[i] = _read_pairs(os.path.join(base, _IC15_STRONG[1].format(i)))
            return lexicons, pairs
    raise ValueError("No lexicon for dataset: {0}, and type: {1}".format(dataset, str(lexicon_type)))


def encode_word(upper_word: str) -> bytes:
    """An upper-cased lexicon word -> its device symbols: ASCII as is, every other code point SENTINEL."""
    if upper_word.isascii():
        return upper_word.encode("ascii")
    return bytes(o if o < 128 else SENTINEL for o in map(ord, upper_word))


def encode_query(rec: str) -> bytes:
    """A recognised word -> its device symbols (upper-cased ASCII).  Refuses non-ASCII text (the sentinel would make it
    equal to any non-ASCII lexicon character) and words longer than MAX_QUERY symbols."""
    if not rec.isascii():
        raise ValueError(f"lexicon queries must be ASCII (strip other characters first, as the writer does): {rec!r}")
    if len(rec) > MAX_QUERY:
        raise ValueError(f"lexicon query of {len(rec)} symbols (max {MAX_QUERY}): {rec[:80]!r}")
    return rec.upper().encode("ascii")


def lexicon_layout(segments: Sequence[Sequence[str]]) -> dict:
    """Upper-cased word lists (one per segment) -> the device layout of glass_lexicon_match as numpy arrays: words
    sorted by length inside each segment (stable: equal lengths keep file order), each starting on a 16-byte boundary;
    word_index = the word's position in the concatenation of the segments in file order, which breaks ties."""
    off, lens, index, seg_off, chunks = [], [], [], [0], []
    pos = nbytes = 0
    for words in segments:
        enc = [encode_word(w) for w in words]
        for j in sorted(range(len(enc)), key=lambda j: len(enc[j])):
            b = enc[j]
            padded = (len(b) + 15) // 16 * 16
            off.append(nbytes)
            lens.append(len(b))
            index.append(pos + j)
            chunks.append(b.ljust(padded, b"\0"))
            nbytes += padded
        pos += len(enc)
        seg_off.append(pos)
    sym = b"".join(chunks) or b"\0" * 16
    if nbytes >= 2 ** 31:
        raise ValueError(f"lexicon of {nbytes} encoded bytes (max 2 GiB)")
    return {"word_off": np.asarray(off, dtype=np.int32), "word_len": np.asarray(lens, dtype=np.int32),
            "word_sym": np.frombuffer(sym, dtype=np.uint8).copy(), "word_index": np.asarray(index, dtype=np.int32),
            "seg_off": np.asarray(seg_off, dtype=np.int32),
            "max_segment_words": max([len(s) for s in segments] or [0])}


class DeviceLexicon:
    """A lexicon encoded once and kept on the device.  `lexicon` is a word list (one segment, key None) or a dict
    {key: word list} such as the per-image strong lexicons of load_lexicon (one segment per key)."""

    def __init__(self, lexicon: Union[Sequence[str], Dict[object, Sequence[str]]], device=None):
        if isinstance(lexicon, dict):
            self.keys = list(lexicon.keys())
            lists = [list(lexicon[k]) for k in self.keys]
        else:
            self.keys = [None]
            lists = [list(lexicon)]
        self._segment = {k: i for i, k in enumerate(self.keys)}
        uppers = [[w.upper() for w in words] for words in lists]         # upper() once: symbols and `pairs` keys
        self.upper = [w for words in uppers for w in words]
        layout = lexicon_layout(uppers)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_segment_words = layout.pop("max_segment_words")
        self.tensors = {k: torch.from_numpy(v).to(self.device) for k, v in layout.items()}

    def __len__(self) -> int:
        return len(self.upper)

    def segment(self, key) -> int:
        """segment number of a key (None for a plain word list); KeyError for an unknown key, as `lexicon[key]`."""
        return self._segment[key]


class LexiconMatcher:
    """`find_match_word(rec, lexicon, pairs)` (lexicon_utils.py:4-28, un-weighted) for many words at once on the
    device: `match(strings, segments)` -> [(pairs[best word upper-cased], distance)], ("", 100) when no word is closer
    than 100.  `lexicon` / `pairs` as load_lexicon returns them (a dict lexicon takes the dict key of each query as its
    segment), or a DeviceLexicon already built from that lexicon.  Only the winner is looked up in `pairs` (KeyError if
    it is missing, as in the reference; the reference also looks up every earlier, larger-distance improvement)."""

    def __init__(self, lexicon, pairs, device=None, weighted_ed: bool = False):
        if weighted_ed:
            raise NotImplementedError(
                "LexiconMatcher is the unit-cost matcher; for the weighted edit distance (LEXICON_WEIGHTED, whose replace "
                "cost is ed_replace_cost, glass/evaluation/lexicon_utils.py:174-180 and its return on :182) use "
                "WeightedLexiconMatcher(lexicon, pairs, text_encoder)")
        self.lexicon = lexicon if isinstance(lexicon, DeviceLexicon) else DeviceLexicon(lexicon, device)
        self.pairs = pairs

    def match(self, strings: Sequence[str], segments: Optional[Sequence[object]] = None) -> List[Tuple[str, int]]:
        from ..ops import native
        keys = list(segments) if segments is not None else [None] * len(strings)
        if len(keys) != len(strings):
            raise ValueError(f"{len(strings)} strings but {len(keys)} segments")
        queries = [encode_query(s) for s in strings]
        seg = [self.lexicon.segment(k) for k in keys]
        t = self.lexicon.tensors
        index, dist = native.lexicon_match(queries, seg, t["word_off"], t["word_len"], t["word_sym"], t["word_index"],
                                           t["seg_off"], self.lexicon.max_segment_words)
        out = []
        for i, d, k in zip(index.cpu().tolist(), dist.cpu().tolist(), keys):
            if i < 0:
                out.append(NO_MATCH)
            else:
                pairs = self.pairs if k is None else self.pairs[k]
                out.append((pairs[self.lexicon.upper[i]], int(d)))
        return out


def symbol_classes(text_encoder) -> Tuple[np.ndarray, List[int]]:
    """-> (sym_class uint8 [256], classes): sym_class[b] = position in `classes` of the class `char_encode` gives the
    device symbol b (an ASCII character as is, SENTINEL for any non-ASCII character), NO_CLASS where it raises KeyError
    (no '[UNK]'); `classes` = the distinct class ids met, ascending.  ValueError unless the character set is ASCII (a
    non-ASCII character of the set would have to be told from the other non-ASCII characters, which share one symbol)."""
    bad = [c for c in text_encoder.dict if len(c) == 1 and ord(c) >= 128]
    if bad:
        raise ValueError(f"the weighted matcher needs an ASCII character set; it holds {bad[:8]!r}")
    ids = {}
    for b in list(range(128)) + [SENTINEL]:
        try:
            ids[b] = int(text_encoder.char_encode(chr(b)))
        except KeyError:
            pass
    classes = sorted(set(ids.values()))
    if not classes or len(classes) >= NO_CLASS:
        raise ValueError(f"{len(classes)} character classes (1..{NO_CLASS - 1})")
    pos = {c: a for a, c in enumerate(classes)}
    table = np.full(256, NO_CLASS, dtype=np.uint8)
    for b, c in ids.items():
        table[b] = pos[c]
    return table, classes


def weighted_cost_tables(rec: str, scores, text_encoder, classes: Sequence[int]):
    """The costs `weighted_edit_distance(rec, word, scores, text_encoder)` adds, as float64 arrays, for m = len(rec):
    del [m] (the query's own character's probability at each step), ins [m] (its mean with the next step's; the last
    step: itself) and rep [m][len(classes)] = max(1 - scores[j][c] / del[j] * 5, 0) for c in `classes` (a pair of
    characters equal up to case costs 0 instead; the caller tests that).  Same operations in the same order as the host
    path, elementwise in float64, so the same bits.
    Raises what the host path raises at its first substitution, before any of it runs: KeyError for a character of `rec`
    without a class, IndexError for fewer score rows than characters, ZeroDivisionError for an own-character probability
    of 0 - and ValueError for a negative or non-finite score (the device orders distances by their bit patterns)."""
    m = len(rec)
    A = len(classes)
    if m == 0:
        return np.zeros(0), np.zeros(0), np.zeros((0, A))
    c1 = [text_encoder.char_encode(ch) for ch in rec]
    S = np.asarray(scores, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError(f"scores of shape {S.shape} ([steps][classes] expected)")
    if m > S.shape[0]:
        raise IndexError(f"{rec!r} has {m} characters but its scores have {S.shape[0]} rows")
    S = S[:m]
    if not (np.isfinite(S).all() and (S >= 0).all()):
        raise ValueError(f"negative or non-finite character probability for {rec!r}")
    own = S[np.arange(m), c1]                                # IndexError for a class beyond the row, as scores[j][c]
    if (own == 0).any():
        raise ZeroDivisionError(f"{rec!r}: probability 0 for its own character at step {int(np.argmax(own == 0))}")
    ins = own.copy()
    ins[:-1] = (own[:-1] + own[1:]) / 2
    with np.errstate(over="ignore"):
        rep = np.maximum(1 - S[:, list(classes)] / own[:, None] * 5, 0)
    return own, ins, rep


class WeightedLexiconMatcher:
    """`find_match_word(rec, lexicon, pairs, scores, weighted_ed=True, text_encoder)` (lexicon_utils.py:26-48, :136-182)
    for many words at once on the device: `match(strings, segments, scores)` -> [(pairs[word], weighted distance)],
    ("", 100) when no candidate is closer than 100; `scores[i]` is record i's `character_probs` ([steps][classes], nested
    lists or an array).  Lexicon, pairs and segments as for LexiconMatcher.  Distances are the host path's float64 values
    bit for bit, and equal distances go to the first word in file order.

    The one place it is stricter than the host path: the errors of `weighted_cost_tables` are raised for every non-empty
    query before anything runs, where the host path meets them at the first substitution it computes (so not at all for a
    query whose candidates are all empty words).  A candidate with a character the encoder has no class for (no '[UNK]')
    raises KeyError after the launch, as `char_encode` does."""

    weighted = True

    def __init__(self, lexicon, pairs, text_encoder, device=None, table_cap_bytes: int = WEIGHTED_TABLE_CAP_BYTES):
        self.lexicon = lexicon if isinstance(lexicon, DeviceLexicon) else DeviceLexicon(lexicon, device)
        self.pairs = pairs
        self.text_encoder = text_encoder
        table, self.classes = symbol_classes(text_encoder)
        self.sym_class = torch.from_numpy(table).to(self.lexicon.device)
        self.table_cap_bytes = int(table_cap_bytes)

    def _chunks(self, sizes: Sequence[int]) -> List[Tuple[int, int]]:
        """[a, b) query ranges whose tables stay under table_cap_bytes (one query at least)"""
        cap = max(self.table_cap_bytes // 8, 1)
        out, a, total = [], 0, 0
        for i, n in enumerate(sizes):
            if i > a and total + n > cap:
                out.append((a, i))
                a, total = i, 0
            total += n
        if len(sizes) > a:
            out.append((a, len(sizes)))
        return out

    def match(self, strings: Sequence[str], segments: Optional[Sequence[object]] = None, scores=None) -> List[Tuple[str, float]]:
        from ..ops import native
        if scores is None:
            raise TypeError("match() needs scores=[character_probs of every string]")
        keys = list(segments) if segments is not None else [None] * len(strings)
        if len(keys) != len(strings):
            raise ValueError(f"{len(strings)} strings but {len(keys)} segments")
        if len(scores) != len(strings):
            raise ValueError(f"{len(strings)} strings but {len(scores)} score tables")
        queries = [encode_query(s) for s in strings]
        seg = [self.lexicon.segment(k) for k in keys]
        tables = []
        for rec, sc in zip(strings, scores):                 # every error of the inputs is raised here, before any launch
            d, i, r = weighted_cost_tables(rec, sc, self.text_encoder, self.classes)
            tables.append(np.concatenate([d, i, r.reshape(-1)]))
        t = self.lexicon.tensors
        index, dist, status = [], [], []
        for a, b in self._chunks([x.size for x in tables]):
            sizes = np.fromiter((x.size for x in tables[a:b]), dtype=np.int64, count=b - a)
            i, d, st = native.lexicon_match_weighted(queries[a:b], seg[a:b], np.concatenate(tables[a:b]), np.cumsum(sizes) - sizes,
                                                     self.sym_class, len(self.classes), t["word_off"], t["word_len"], t["word_sym"],
                                                     t["word_index"], t["seg_off"], self.lexicon.max_segment_words)
            index += i.cpu().tolist()
            dist += d.cpu().tolist()
            status += st.cpu().tolist()
        for q, st in enumerate(status):
            if st & 2:
                raise RuntimeError(f"glass_lexicon_match_weighted refused the tables of query {q} ({strings[q]!r})")
            if st & 1:
                raise KeyError(f"[UNK]: a candidate of {strings[q]!r} holds a character the text encoder has no class for")
        out = []
        for i, d, k, s in zip(index, dist, keys, strings):
            if i < 0:
                out.append(NO_MATCH)
            else:
                pairs = self.pairs if k is None else self.pairs[k]
                word = self.lexicon.upper[i]
                # the DP returns its integer border untouched when either word is empty, as the host path does
                out.append((pairs[word], int(d) if (not s or not word) else d))
        return out


NO_FOLD_TOKENS = ("[GO]", "[s]", "[UNK]", "[blank]")
MAX_FOLD = 256                # fold symbols of a trie (8 mask words of 32 bits per node)


def fold_table(characters: Sequence[str], eos: int, case_insensitive: bool = True) -> Tuple[np.ndarray, List[str]]:
    """-> (fold int32 [C], symbols): fold[c] = the fold symbol of class c, numbered densely in class order, and the fold
    symbols' strings.  The fold symbol of a class is its character upper-cased with `str.upper()` where that is one
    character (else, and with case_insensitive=False, the character itself); -1 for the special tokens, any other
    multi-character class and the class `eos`."""
    fold = np.full(len(characters), -1, dtype=np.int32)
    ids: Dict[str, int] = {}
    for c, ch in enumerate(characters):
        if c == eos or ch in NO_FOLD_TOKENS or len(ch) != 1:
            continue
        up = ch.upper() if case_insensitive else ch
        sym = up if len(up) == 1 else ch
        fold[c] = ids.setdefault(sym, len(ids))
    if not 1 <= len(ids) <= MAX_FOLD:
        raise ValueError(f"{len(ids)} fold symbols (1..{MAX_FOLD})")
    return fold, list(ids)


class LexiconTrie:
    """A lexicon as a trie over the decoder's classes, built once on the host and kept on the device: what
    glass_beam_search_lexicon consults at every decoding step (include/glass_hip_ext.h has the layout).

    `lexicon`: a word list (one segment, key None) or a dict {key: word list} (one segment per key), as DeviceLexicon takes
    them; `text_encoder_or_characters`: a TextEncoder or its list of class strings; `max_len`: the decoder's steps (a word
    needs one more step than it has characters, for the stop); `eos`: the stop class.  Words are folded as the matchers fold
    them - `upper()` once at load - or taken as they are with case_insensitive=False; `upper[i]` is word i (position in the
    concatenation of the segments in file order) upper-cased, as in DeviceLexicon.  A word that is empty, longer than
    max_len - 1 characters or holds a character without a fold symbol is left out and counted in `skipped`; so every node
    has a word below it and a hypothesis alive at the last step can only stop.

    numpy arrays (nodes in breadth-first order, a node's children contiguous and ordered by fold symbol): `fold` int32 [C],
    `child_mask` uint32 [N,MW], `child_base` int32 [N], `node_word` int32 [N] (-1, or the first word that ends there),
    `seg_root` int32 [S] (-1 = an empty segment); child(node, f) = child_base[node] + popcount(mask bits below f).
    `word_node` int32 [len(upper)] (host only): the node every word ends at, -1 for a word that was left out.
    `tensors` holds them on the device (the mask as int32 bit patterns) with the int "F"."""

    def __init__(self, lexicon: Union[Sequence[str], Dict[object, Sequence[str]]], text_encoder_or_characters, max_len: int,
                 eos: int, case_insensitive: bool = True, device=None):
        import time
        t0 = time.perf_counter()
        if isinstance(lexicon, dict):
            self.keys = list(lexicon.keys())
            lists = [list(lexicon[k]) for k in self.keys]
        else:
            self.keys = [None]
            lists = [list(lexicon)]
        self._segment = {k: i for i, k in enumerate(self.keys)}
        characters = list(getattr(text_encoder_or_characters, "character", text_encoder_or_characters))
        self.num_classes, self.max_len, self.eos = len(characters), int(max_len), int(eos)
        self.case_insensitive = bool(case_insensitive)
        if not 0 <= self.eos < self.num_classes:
            raise ValueError(f"eos {eos} outside [0, {self.num_classes})")
        self.fold, self.fold_symbols = fold_table(characters, self.eos, self.case_insensitive)
        self.num_fold = F = len(self.fold_symbols)
        self.mask_words = MW = (F + 31) // 32
        uppers = [[w.upper() for w in words] for words in lists]
        self.upper = [w for words in uppers for w in words]
        self.segment_sizes = [len(words) for words in lists]      # words per segment, left-out ones included: `upper` in slices
        folded = uppers if self.case_insensitive else lists
        sym_id = {s: i for i, s in enumerate(self.fold_symbols)}
        self.skipped = {"empty": 0, "too_long": 0, "no_class": 0}
        # ---- the kept words as rows of fold symbols
        w_seg, w_idx, w_sym = [], [], []
        pos = 0
        for seg, words in enumerate(folded):
            for j, w in enumerate(words):
                if not w:
                    self.skipped["empty"] += 1
                elif len(w) > self.max_len - 1:
                    self.skipped["too_long"] += 1
                else:
                    ids = [sym_id.get(ch, -1) for ch in w]
                    if min(ids) < 0:
                        self.skipped["no_class"] += 1
                    else:
                        w_seg.append(seg); w_idx.append(pos + j); w_sym.append(ids)
            pos += len(words)
        S, W = len(lists), len(w_sym)
        w_len = np.fromiter((len(v) for v in w_sym), dtype=np.int64, count=W)
        depth = int(w_len.max()) if W else 0
        sym = np.full((W, max(depth, 1)), -1, dtype=np.int64)
        for i, v in enumerate(w_sym):
            sym[i, :len(v)] = v
        w_seg = np.asarray(w_seg, dtype=np.int64)
        w_idx = np.asarray(w_idx, dtype=np.int64)
        # ---- level by level: the nodes of depth d + 1 are the distinct (parent, symbol) pairs, in that order
        self.seg_root = np.full(S, -1, dtype=np.int32)
        used = np.unique(w_seg)
        self.seg_root[used] = np.arange(len(used), dtype=np.int32)
        n = len(used)
        at = self.seg_root[w_seg].astype(np.int64) if W else np.zeros(0, dtype=np.int64)       # node of every word's prefix
        masks, bases, words_at = [np.zeros((n, MW), dtype=np.uint32)], [np.zeros(n, dtype=np.int64)], [np.full(n, -1, dtype=np.int64)]
        level0 = 0
        for d in range(depth):
            live = np.nonzero(w_len > d)[0]
            key, inv = np.unique(at[live] * F + sym[live, d], return_inverse=True)
            parent, f = key // F - level0, key % F
            child = n + np.arange(len(key), dtype=np.int64)
            np.bitwise_or.at(masks[-1], (parent, f >> 5), (np.uint32(1) << (f & 31).astype(np.uint32)))
            first = np.unique(parent, return_index=True)
            bases[-1][first[0]] = child[first[1]]
            at[live] = child[inv.reshape(-1)]
            end = live[w_len[live] == d + 1]
            ends = np.full(len(key), np.iinfo(np.int64).max, dtype=np.int64)
            np.minimum.at(ends, at[end] - n, w_idx[end])
            ends[ends == np.iinfo(np.int64).max] = -1
            level0, n = n, n + len(key)
            masks.append(np.zeros((len(key), MW), dtype=np.uint32)); bases.append(np.zeros(len(key), dtype=np.int64)); words_at.append(ends)
        if n == 0:                  # no word at all: one node that no root points to, so that no array is empty
            masks, bases, words_at, n = [np.zeros((1, MW), dtype=np.uint32)], [np.zeros(1, dtype=np.int64)], [np.full(1, -1, dtype=np.int64)], 1
        if n >= 2 ** 31:
            raise ValueError(f"lexicon trie of {n} nodes (max 2^31 - 1)")
        self.num_nodes = n
        # the node every word ends at (indexed as `upper`; -1 for a word that was left out): what a word prior is attached to
        self.word_node = np.full(len(self.upper), -1, dtype=np.int32)
        self.word_node[w_idx] = at
        self.child_mask = np.ascontiguousarray(np.concatenate(masks))
        self.child_base = np.concatenate(bases).astype(np.int32)
        self.node_word = np.concatenate(words_at).astype(np.int32)
        self.nbytes = int(self.child_mask.nbytes + self.child_base.nbytes + self.node_word.nbytes + self.seg_root.nbytes + self.fold.nbytes)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.tensors = {"child_mask": torch.from_numpy(self.child_mask.view(np.int32)).to(self.device),
                        "child_base": torch.from_numpy(self.child_base).to(self.device),
                        "node_word": torch.from_numpy(self.node_word).to(self.device),
                        "seg_root": torch.from_numpy(self.seg_root).to(self.device),
                        "fold": torch.from_numpy(self.fold).to(self.device), "F": F}
        self.build_seconds = time.perf_counter() - t0

    def __len__(self) -> int:
        return len(self.upper)

    def segment(self, key) -> int:
        """segment number of a key (None for a plain word list); KeyError for an unknown key, as `lexicon[key]`."""
        return self._segment[key]
