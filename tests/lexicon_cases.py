"""Seeded synthetic lexicons and queries for the lexicon-matching tests (tests/test_lexicon.py, tests/test_gpu_lexicon.py).

The MaskTextSpotterV3 lexicon files are not redistributable here, so every case is generated from a fixed seed with
Python's `random.Random` (its sequence for a given seed is stable across Python versions).  The random case is large
enough that the host `find_match_word` needs minutes for it, so its answers are recorded in
tests/golden/lexicon_random.json together with a digest of the generated words; the CPU test re-derives a sample of
them with `find_match_word`.  Regenerate with `python tests/lexicon_cases.py` (uses every core).
"""
import hashlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_RANDOM = os.path.join(ROOT, "tests", "golden", "lexicon_random.json")

_ASCII = "abcdefghABCDEFGH0123-'."
_NON_ASCII = "éßﬁΩöİ"          # é/ö/Ω stay non-ASCII upper-cased, ß -> SS and ﬁ -> FI change the length, İ stays one code point


def _rand_word(r: random.Random, n: int, non_ascii: float = 0.03) -> str:
    return "".join(r.choice(_NON_ASCII) if r.random() < non_ascii else r.choice(_ASCII) for _ in range(n))


def _word_length(r: random.Random) -> int:
    u = r.random()
    return r.randint(0, 10) if u < 0.7 else r.randint(11, 24) if u < 0.9 else r.randint(25, 70)


def random_case(n_words: int = 5000, n_queries: int = 512, seed: int = 20261016):
    """(lexicon, pairs, queries): words of 0-70 symbols with case variants, duplicates and non-ASCII characters;
    ASCII queries of 0-64 symbols: exact hits, near hits (1-3 edits of a word) and unrelated strings."""
    r = random.Random(seed)
    lexicon = []
    for _ in range(n_words):
        u = r.random()
        if lexicon and u < 0.08:
            lexicon.append(r.choice(lexicon))                                  # duplicate
        elif lexicon and u < 0.16:
            lexicon.append(r.choice(lexicon).swapcase())                       # case variant
        else:
            lexicon.append(_rand_word(r, _word_length(r)))
    pairs = {w.upper(): w for w in lexicon}
    queries = []
    for i in range(n_queries):
        u = r.random()
        if i < 4:
            q = ["", "A" * 64, _rand_word(r, 64, 0.0), "b"][i]
        elif u < 0.35:
            q = "".join(c for c in r.choice(lexicon) if ord(c) < 128)         # exact hit (up to the non-ASCII strip)
        elif u < 0.7:
            q = list("".join(c for c in r.choice(lexicon) if ord(c) < 128))
            for _ in range(r.randint(1, 3)):
                k = r.randint(0, len(q))
                op = r.randint(0, 2)
                if op == 0:
                    q.insert(k, r.choice(_ASCII))
                elif q and op == 1:
                    q[min(k, len(q) - 1)] = r.choice(_ASCII)
                elif q:
                    del q[min(k, len(q) - 1)]
            q = "".join(q)
        else:
            q = _rand_word(r, r.randint(0, 64), 0.0)
        queries.append(q[:64] if r.random() < 0.5 else q[:64].lower())
    return lexicon, pairs, queries


def case_digest(lexicon, queries) -> str:
    h = hashlib.sha256()
    for w in lexicon + ["\0"] + queries:
        h.update(w.encode("utf-8") + b"\n")
    return h.hexdigest()[:16]


def load_random_golden():
    with open(GOLDEN_RANDOM) as f:
        g = json.load(f)
    return g["digest"], [tuple(x) for x in g["expected"]]


def ties_case(n_words: int = 200_000, seed: int = 7):
    """(lexicon, pairs, queries) for equal minima over many workgroups: a background of words over letters no query
    uses, with words at distance 1 from 'HELLO' planted in file order against their length order (the first one in file
    order is longer than later ones, so it sorts after them on the device), plus queries with natural ties."""
    r = random.Random(seed)
    lexicon = ["".join(r.choice("QRSTUVWXYZ") for _ in range(r.randint(1, 6))) for _ in range(n_words)]
    for pos, w in ((60_123, "HELLOQ"), (61_000, "HELL"), (150_000, "ELLO"), (199_990, "HXLLO"), (130_000, "hello!")):
        lexicon[pos] = w
    pairs = {w.upper(): w.lower() for w in lexicon}
    return lexicon, pairs, ["HELLO", "hello", "QRS", "", "ZZZZZZ"]


def segments_case(seed: int = 11):
    """(lexicons {1..50: words}, pairs {1..50: dict}, queries [(text, image id)]): image 17 has an empty lexicon, image 33
    only words that every query of <= 64 symbols is at least 100 away from: 164-220 symbols over X, Y, Z (rejected by
    length alone) and 100-163 over Y, Z (fully computed, then rejected)."""
    r = random.Random(seed)
    lexicons, pairs = {}, {}
    for i in range(1, 51):
        if i == 17:
            words = []
        elif i == 33:
            words = ["".join(r.choice("XYZ") for _ in range(r.randint(164, 220))) for _ in range(20)]
            words += ["".join(r.choice("YZ") for _ in range(r.randint(100, 163))) for _ in range(20)]
            r.shuffle(words)
        else:
            words = [_rand_word(r, r.randint(1, 14)) for _ in range(r.randint(60, 140))]
        lexicons[i] = words
        pairs[i] = {w.upper(): w for w in words}
    queries = []
    for k in range(400):
        img = [17, 33, 33][k] if k < 3 else r.randint(1, 50)
        words = lexicons[img]
        if k == 1:
            q = "X" * 64
        elif k == 2:
            q = ""
        elif words and r.random() < 0.6:
            q = "".join(c for c in r.choice(words) if ord(c) < 128)[:64]
        else:
            q = _rand_word(r, r.randint(0, 20), 0.0)
        queries.append((q, img))
    return lexicons, pairs, queries


def _one(args):
    sys.path.insert(0, os.path.join(ROOT, "glass-text-spotting_amd"))
    from glass_amd.evaluation.text_evaluator import find_match_word
    q, lexicon, pairs = args
    return find_match_word(q, lexicon, pairs)


def write_random_golden() -> None:
    import multiprocessing
    lexicon, pairs, queries = random_case()
    with multiprocessing.Pool() as pool:
        expected = pool.map(_one, [(q, lexicon, pairs) for q in queries], chunksize=4)
    with open(GOLDEN_RANDOM, "w") as f:
        json.dump({"what": "find_match_word(q, lexicon, pairs) for random_case() of tests/lexicon_cases.py",
                   "digest": case_digest(lexicon, queries), "expected": [list(x) for x in expected]}, f, ensure_ascii=False)
        f.write("\n")


if __name__ == "__main__":
    write_random_golden()
    print("wrote", GOLDEN_RANDOM)
