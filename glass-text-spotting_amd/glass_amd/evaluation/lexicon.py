"""Lexicons for lexicon-constrained text evaluation (reference glass/evaluation/lexicon_utils.py).

  * `load_lexicon` - `get_lexicon` (:51-131): the MaskTextSpotterV3 lexicon files, with `root` standing in for the
    directory the reference hard-codes; returns (lexicon, pairs) in the shapes `TextResultWriter` takes.
  * `DeviceLexicon` - a word list, or a dict of per-image word lists (one segment each), upper-cased and encoded once
    and kept on the device.
  * `LexiconMatcher` - `find_match_word` (:4-28, the un-weighted branch) for a whole batch of recognised words in one
    launch of glass_lexicon_match (csrc/lexicon.hip); `TextResultWriter(matcher=...)` uses it.

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
                "weighted edit distance (LEXICON_WEIGHTED) is not built: upstream it cannot run - ed_replace_cost "
                "(glass/evaluation/lexicon_utils.py:174-180) has no return, so any substitution adds None (TypeError)")
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
