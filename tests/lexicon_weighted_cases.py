"""Seeded synthetic cases for the weighted lexicon matcher (tests/test_lexicon_weighted.py, tests/test_gpu_lexicon_weighted.py,
scripts/make_lexicon_weighted_golden.py).

Everything comes from `random.Random` with a fixed seed (its sequence is stable across Python versions).  A score row is
float32(w / sum(w)) of integer weights w: integers and one IEEE division round the same everywhere, `exp` does not.  Some
weights of characters other than the query's own are 0 (a substitution into them costs exactly 1.0), the own character's
weight never is (it is the divisor).  Every case is (lexicon, pairs, queries, scores, encoder); a dict lexicon has one
word list per image and its queries are (text, image) pairs.

The reference's answers for `random_case`, `ties_case` and `far_case` are recorded in tests/golden/lexicon_weighted.json
(scripts/make_lexicon_weighted_golden.py) with a digest of the generated inputs.
"""
import functools
import hashlib
import json
import os
import random
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lexicon_weighted.json")

CHARSET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ "
_ASCII = "abcdefghABCDEFGH0123-'."
_NON_ASCII = "éßﬁΩöİ"          # é/ö/Ω stay non-ASCII upper-cased, ß -> SS and ﬁ -> FI change the length


class Encoder:
    """the two methods and the table of the recogniser's TextEncoder that the weighted distance uses"""

    def __init__(self, charset: str = CHARSET, unk: bool = True):
        self.character = ["[GO]", "[s]"] + (["[UNK]"] if unk else []) + list(charset)
        self.dict = {c: i for i, c in enumerate(self.character)}

    def char_encode(self, char: str) -> int:
        assert len(char) == 1
        return self.dict[char] if char in self.dict else self.dict["[UNK]"]


def _f32_row(weights):
    total = sum(weights)
    n = len(weights)
    return list(struct.unpack(f"<{n}f", struct.pack(f"<{n}f", *[w / total for w in weights])))


def score_table(r: random.Random, rec: str, enc: Encoder, rows: int, zero: float = 0.5, own=(30, 400), other=(1, 40)):
    """[rows][classes] probabilities for the recognised word `rec`: row j favours rec[j]'s class"""
    C = len(enc.character)
    table = []
    for j in range(rows):
        w = [0 if r.random() < zero else r.randint(*other) for _ in range(C)]
        k = enc.char_encode(rec[j]) if j < len(rec) else r.randrange(C)
        w[k] = r.randint(*own)
        table.append(_f32_row(w))
    return table


def _rand_word(r: random.Random, n: int, non_ascii: float = 0.03) -> str:
    return "".join(r.choice(_NON_ASCII) if r.random() < non_ascii else r.choice(_ASCII) for _ in range(n))


def _strip(w: str) -> str:
    return "".join(c for c in w if ord(c) < 128)


def _edit(r: random.Random, w: str, edits: int) -> str:
    q = list(w)
    for _ in range(edits):
        k = r.randint(0, len(q))
        op = r.randint(0, 2)
        if op == 0:
            q.insert(k, r.choice(_ASCII))
        elif q and op == 1:
            q[min(k, len(q) - 1)] = r.choice(_ASCII)
        elif q:
            del q[min(k, len(q) - 1)]
    return "".join(q)


@functools.lru_cache(maxsize=None)
def random_case(n_words: int = 4000, n_queries: int = 256, seed: int = 20261018):
    """256 queries against 4,000 words: word lengths 0-70 with duplicates, case variants and non-ASCII characters; queries
    of 0-24 symbols (a few up to 64, with 65 score rows), exact, near and unrelated, in mixed case; an encoder with [UNK]."""
    r = random.Random(seed)
    enc = Encoder()
    lexicon = []
    for _ in range(n_words):
        u = r.random()
        if lexicon and u < 0.08:
            lexicon.append(r.choice(lexicon))
        elif lexicon and u < 0.16:
            lexicon.append(r.choice(lexicon).swapcase())
        else:
            v = r.random()
            lexicon.append(_rand_word(r, r.randint(0, 10) if v < 0.7 else r.randint(11, 24) if v < 0.93 else r.randint(25, 70)))
    pairs = {w.upper(): w for w in lexicon}
    queries, scores = [], []
    for i in range(n_queries):
        u = r.random()
        if i < 4:
            q = ["", _rand_word(r, 64, 0.0), "b", "A" * 64][i]
        elif i < 12:
            q = _edit(r, _strip(r.choice([w for w in lexicon if len(w) > 40])), r.randint(0, 4))[:64]
        elif u < 0.3:
            q = _strip(r.choice(lexicon))[:24]
        elif u < 0.7:
            q = _edit(r, _strip(r.choice(lexicon)), r.randint(1, 3))[:24]
        else:
            q = _rand_word(r, r.randint(0, 24), 0.0)
        q = "".join(c.swapcase() if r.random() < 0.3 else c for c in q)
        queries.append(q)
        scores.append(score_table(r, q, enc, 26 if len(q) <= 25 else 65, zero=r.choice([0.3, 0.6, 0.9])))
    return lexicon, pairs, queries, scores, enc


TIES_WINNERS = {"hello": "helloq", "world": "worla", "tiger": "txger"}


@functools.lru_cache(maxsize=None)
def ties_case(n_words: int = 12_000, seed: int = 7):
    """Exact ties between planted words over a background no query is near (letters no query uses, 3-7 symbols):
      'hello': HELLOQ (one insertion at the end, cost own[4]) at 3,000 and HELL (one deletion at the end, cost own[4]) at 9,500:
               the first in file order is the longer word, so it sorts after the other on the device; HELLX and HEXLO cost
               exactly 1.0 (X has weight 0 there), more than own[4] < 1;
      'world': WORLA at 2,000 and WORLD at 9,000 both cost 0.0 (p(A) >= p(d) / 5 at the last step clamps to 0);
      'tiger': TXGER at 1,500 and TIGEX at 8,000 both cost exactly 1.0 (X has weight 0 at both steps), nothing is closer.
    Equal-length planted words are more than 1,024 words of their length apart, i.e. in different workgroups."""
    r = random.Random(seed)
    enc = Encoder()
    lexicon = ["".join(r.choice("QSUVYZJKPM") for _ in range(r.randint(3, 7))) for _ in range(n_words)]
    for pos, w in ((3_000, "HelloQ"), (9_500, "hell"), (5_000, "HELLX"), (7_000, "hexlo"),
                   (2_000, "WORLA"), (9_000, "world"), (1_500, "Txger"), (8_000, "TIGEX")):
        lexicon[pos] = w
    pairs = {w.upper(): w.lower() for w in lexicon}
    queries = ["hello", "world", "tiger", "", "QSU", "zzzzzz"]
    C = len(enc.character)
    scores = []
    for q in queries:
        table = []
        for j in range(26):
            w = [0] * C
            for c in "abcdefghijklmnopqrstuvwyz":                       # no weight on 'x' / 'X' anywhere
                w[enc.char_encode(c)] = r.randint(1, 3)
            if j < len(q):
                w[enc.char_encode(q[j])] = 400
            if q == "world" and j == 4:
                w[enc.char_encode("A")] = 100                            # 100 / 400 * 5 > 1: the substitution is free
            table.append(_f32_row(w))
        scores.append(table)
    return lexicon, pairs, queries, scores, enc


@functools.lru_cache(maxsize=None)
def crowd_case(n_words: int = 3000, seed: int = 13):
    """1- and 2-symbol queries against 3,000 words of 0-3 symbols: most of the segment is a candidate (more than 1,024, over
    several chunks and every wave), with many repeated words (the first occurrence counts)."""
    r = random.Random(seed)
    enc = Encoder()
    alphabet = "abcdefABCDEF0123"
    lexicon = ["".join(r.choice(alphabet) for _ in range(r.choice([0, 1, 2, 2, 3, 3, 3]))) for _ in range(n_words)]
    pairs = {w.upper(): w + "!" for w in lexicon}
    queries = ["a", "B", "ab", "Fe", "z", "zz", "0", "c3"]
    scores = [score_table(r, q, enc, 26, zero=0.4, own=(5, 60), other=(1, 30)) for q in queries]
    return lexicon, pairs, queries, scores, enc


@functools.lru_cache(maxsize=None)
def far_case(seed: int = 17):
    """dist_min_pre stays 100: image 1 and image 2 hold words of 164-166 symbols that contain the 64-symbol query as a
    subsequence (unit distance = 100..102 exactly) and words of those lengths that do not (farther than 102).  Image 1's
    query has own-character probabilities well below 1, so ~100 insertions cost far less than 100 and a match is found;
    image 2's has probability exactly 1.0 for its own characters, every insertion costs 1.0, and none is found."""
    r = random.Random(seed)
    enc = Encoder()
    query = "".join(r.choice("abcdefghABCDEFGH") for _ in range(64))
    lexicons, pairs = {}, {}
    for img in (1, 2):
        words = []
        for k in range(36):
            w = list(query.upper())
            for _ in range(100 + k % 3):
                w.insert(r.randint(0, len(w)), r.choice("XYZ"))
            words.append("".join(w))
        words += ["".join(r.choice("XYZ") for _ in range(164 + k % 3)) for k in range(12)]
        r.shuffle(words)
        lexicons[img] = words
        pairs[img] = {w.upper(): f"w{img}_{k}" for k, w in enumerate(words)}
    C = len(enc.character)
    peaked = []
    for j in range(65):
        w = [0] * C
        w[enc.char_encode(query[j]) if j < 64 else 0] = 7                # float32(7 / 7) = 1.0
        peaked.append(_f32_row(w))
    queries = [(query, 1), (query, 2)]
    scores = [score_table(r, query, enc, 65, zero=0.2, own=(60, 200), other=(1, 12)), peaked]
    return lexicons, pairs, queries, scores, enc


@functools.lru_cache(maxsize=None)
def segments_case(seed: int = 11):
    """30 per-image lexicons: image 7 is empty, image 9 holds only the empty word, image 21 holds a 200-symbol word, which
    the length filter alone rejects for any query (a candidate is at most 64 + 102 = 166 symbols long: its unit distance is
    at least its excess length), beside the longest word that can be a candidate: 166 symbols containing the 64-symbol query
    (unit distance 102, dist_min_pre 100 from a 164-symbol one)."""
    r = random.Random(seed)
    enc = Encoder()
    long_query = "".join(r.choice("abcdABCD") for _ in range(64))

    def stretch(n):
        w = list(long_query.upper())
        while len(w) < n:
            w.insert(r.randint(0, len(w)), r.choice("XYZ"))
        return "".join(w)

    lexicons, pairs = {}, {}
    for i in range(1, 31):
        if i == 7:
            words = []
        elif i == 9:
            words = [""]
        elif i == 21:
            words = [stretch(200), stretch(166), stretch(164), "X" * 165]
        else:
            words = [_rand_word(r, r.randint(1, 14)) for _ in range(r.randint(40, 90))]
        lexicons[i] = words
        pairs[i] = {w.upper(): f"{i}:{w}" for w in words}
    queries, scores = [], []
    for k in range(120):
        img = [7, 9, 9, 21, 21][k] if k < 5 else r.choice([i for i in range(1, 31) if i != 21])
        words = lexicons[img]
        if k < 5:
            q = ["word", "abc", "", long_query, "abcd"][k]
        elif words and words != [""] and r.random() < 0.6:
            q = _edit(r, _strip(r.choice(words)), r.randint(0, 2))[:24]
        else:
            q = _rand_word(r, r.randint(0, 20), 0.0)
        queries.append((q, img))
        scores.append(score_table(r, q, enc, 65 if len(q) > 25 else 26, zero=0.5, own=(20, 100), other=(1, 10)))
    return lexicons, pairs, queries, scores, enc


@functools.lru_cache(maxsize=None)
def no_unk_case(seed: int = 19):
    """an encoder WITHOUT [UNK] over a lexicon with one word outside its character set ('CAFÉ'): a query near it meets
    char_encode's KeyError, a query it is no candidate of does not"""
    r = random.Random(seed)
    enc = Encoder(unk=False)
    lexicon = ["apple", "maple", "café", "orange", "grape"]
    pairs = {w.upper(): w for w in lexicon}
    queries = ["cafe", "orange"]
    scores = [score_table(r, q, enc, 26) for q in queries]
    return lexicon, pairs, queries, scores, enc


@functools.lru_cache(maxsize=None)
def wide_case(seed: int = 23):
    """an encoder over all 128 ASCII characters and [UNK] (129 classes): a 64-symbol query's substitution table is 64 x 129
    doubles, past what the workgroup keeps in LDS"""
    r = random.Random(seed)
    enc = Encoder("".join(chr(i) for i in range(128)))
    lexicon = [_rand_word(r, r.choice([3, 5, 8, 30, 60, 64, 66])) for _ in range(300)]
    pairs = {w.upper(): w for w in lexicon}
    queries = [_edit(r, _strip(lexicon[k]), 2)[:64] for k in (5, 17, 40, 99, 123, 250)] + [_strip(lexicon[200])[:64], "A" * 64]
    scores = [score_table(r, q, enc, 65, zero=0.5) for q in queries]
    return lexicon, pairs, queries, scores, enc


def case_digest(lexicon, queries, scores) -> str:
    """sha256[:16] over the words, the queries and the bits of every score"""
    h = hashlib.sha256()
    lists = [lexicon[k] for k in lexicon] if isinstance(lexicon, dict) else [lexicon]
    for words in lists:
        for w in words:
            h.update(w.encode("utf-8") + b"\n")
        h.update(b"\0")
    for q in queries:
        h.update(repr(q).encode("utf-8") + b"\n")
    for table in scores:
        for row in table:
            h.update(struct.pack(f"<{len(row)}d", *row))
    return h.hexdigest()[:16]


GOLDEN_CASES = {"random": random_case, "ties": ties_case, "far": far_case}


def load_golden():
    """{case: (digest, [(word, float.hex(distance)), ...])}"""
    with open(GOLDEN) as f:
        g = json.load(f)
    return {name: (g["digest"][name], [tuple(x) for x in g["expected"][name]]) for name in GOLDEN_CASES}


def host_queries(case):
    """the case's queries as find_match_word_weighted arguments: [(rec, lexicon, pairs, scores)]"""
    lexicon, pairs, queries, scores, _ = case
    out = []
    for q, sc in zip(queries, scores):
        if isinstance(lexicon, dict):
            out.append((q[0], lexicon[q[1]], pairs[q[1]], sc))
        else:
            out.append((q, lexicon, pairs, sc))
    return out


def as_hex(result):
    word, dist = result
    return word, float(dist).hex()
