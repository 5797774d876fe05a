"""The cases of the pattern-constrained beam search (evaluation/pattern.py, glass_beam_search_dfa), for tests/test_pattern.py
(CPU) and tests/test_gpu_pattern_beam.py.

Expected values owe nothing to the regex compiler: a case's language {w : re.fullmatch(regex, w), 1 <= |w| <= L - 1} is
ENUMERATED (candidate strings from the case's own generator, every one judged by `re.fullmatch`) and handed as a lexicon to
the float64 replay of tests/lexicon_beam_cases.py, which knows tries of words only.  A trie node at depth t has, by
construction, a word of at most L - 1 characters below it - which is the decoding rule "t + 1 + dist[q'] <= L - 1" of
evaluation/pattern.py stated on the enumerated language.
"""
import itertools
import re

import beam_cases as BC
import lexicon_beam_cases as LC

MARGIN, TOL = LC.MARGIN, LC.TOL

# ------------------------------------------------------------------ the compiler against re.fullmatch
SMALL = ["[GO]", "[s]", "a", "b", "1", "-", "A", "B"]          # a small character set: every string up to length 5 is checked
SMALL_ALPHABET = [c for c in SMALL if len(c) == 1]
REGEXES = [
    r"a", r"ab", r"a|b", r"ab|a", r"ab|a1|abb",                  # literals, | with a shared prefix
    r"(ab|a)b?", r"(a|b)*1", r"((a|b)(1|-))+", r"(a(b(1)?)?)?-",  # groups, nested groups
    r"(?:a|b){2,}", r"(?:ab)+", r"a||b", r"(a|)b",               # non-capturing groups, empty branches
    r"[ab]+", r"[^a]", r"[^ab1]*", r"[a\-]+", r"[]a]", r"[a-b1]{2}", r"[A-B]+1?", r"[--1]",   # classes, ranges, negation
    r"[xyz]a?", r"[^\w\-]b",                                     # a class that is empty over this set
    r".", r".{2}", r".*b",                                       # any character
    r"\d+", r"\w-\w", r"\D\S", r"[\d\-]+", r"\W", r"a\s?b", r"[^\d]a",   # class escapes
    r"a\-b", r"\-+",                                             # escaped literals
    r"a*", r"a+b", r"a?b", r"a{2}", r"a{2,}", r"a{0,2}b", r"a{1,3}", r"(ab){0,2}", r"(a|b){3}", r"a{,2}",   # quantifiers
]
UNSUPPORTED = [r"^a", r"a$", r"(a)\1", r"(?=a)b", r"(?!a)b", r"(?<=a)b", r"(?<!a)b", r"a*?", r"a+?", r"a??", r"a{1,2}?", r"a*+",
               r"a++", r"(?P<n>a)", r"(?P=n)", r"(?i)a", r"(?#c)a", r"a\b", r"\Aa", r"a\Z", r"*a", r"a{2", r"(a", r"a)", r"[a", r"a{3,2}",
               r"[b-a]", r"\n", "a\\"]


def strings_up_to(alphabet, n):
    for m in range(n + 1):
        for w in itertools.product(alphabet, repeat=m):
            yield "".join(w)


def bfs_dist(nxt, accept):
    """fewest symbols from every state to an accepting one, by a breadth-first search backwards from the accepting states
    over the unpacked transitions; None where there is no path"""
    N = len(accept)
    back = [[] for _ in range(N)]
    for q in range(N):
        for e in nxt[q]:
            if e >= 0:
                back[int(e) & 0xFFFFFF].append(q)
    dist = [None] * N
    level = [q for q in range(N) if accept[q] >= 0]
    for q in level:
        dist[q] = 0
    d = 0
    while level:
        d += 1
        new = []
        for q in level:
            for p in back[q]:
                if dist[p] is None:
                    dist[p] = d
                    new.append(p)
        level = new
    return dist


# ------------------------------------------------------------------ the search cases
C13 = ["[GO]", "[s]", "a", "b", "c", "0", "1", "2", "3", "4", "-", "A", "B"]      # eos = 1


def _product(alphabet, lo, hi):
    return lambda: ("".join(w) for n in range(lo, hi + 1) for w in itertools.product(alphabet, repeat=n))


def _plates():
    up = [chr(ord("A") + i) for i in range(26)]
    return (a + b + "".join(d) for a in up for b in up for n in (2, 3) for d in itertools.product("0123456789", repeat=n))


def _hi_chars():
    ch = LC.generic_characters(256)
    return [ch[2], ch[3], ch[130], ch[254], ch[255]]


# name -> dict(B k T L C eos seed chars ci patterns item_keys candidates fc_scale boost).  `patterns`: one regex or {key: regex};
# item_keys: the segment key of every item (an int that is no key: a segment number out of range, given as is); `candidates`:
# {key: generator of a superset of the segment's language} - strings over the characters the regex can match at all, up to
# L - 1 of them; `boost`: added to the output layer's bias of these classes, so that a search forced along them keeps |score|
# small (float32 rounding of the running sum grows with it; see lexicon_beam_cases.CASES on fc_scale.  l64_a63 without it: 64
# forced steps reach scores of -343 and -584, where one float32 unit is 3e-5 / 6e-5 and the running sum alone is 3.8e-4 off).
# Seeds: the first of 100.. for which every item's gaps in the float64 replay exceed MARGIN (test_pattern.py asserts it).
CASES = {
    "greedy_k1_c13_l4": dict(B=3, k=1, T=7, L=4, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"[ab]+", item_keys=[None] * 3,
                             candidates={None: _product("abc", 1, 3)}),
    "digits_l4_k5": dict(B=3, k=5, T=7, L=4, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"\d+", item_keys=[None] * 3,
                         candidates={None: _product("01234a-", 1, 3)}),
    "too_long_for_l4": dict(B=2, k=3, T=7, L=4, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"ab{3,}", item_keys=[None] * 2,
                            candidates={None: _product("ab", 1, 3)}),
    "plates_c97_l26_t32_k3": dict(B=2, k=3, T=32, L=26, C=97, eos=1, seed=100, chars="shipped", ci=True, patterns=r"[A-Z]{2}\d{2,3}",
                                  item_keys=[None] * 2, candidates={None: _plates}, fc_scale=0.25),
    "shared_prefix_k4": dict(B=3, k=4, T=7, L=6, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"(ab|a)c?", item_keys=[None] * 3,
                             candidates={None: _product("abc", 1, 5)}),
    "star_k4": dict(B=3, k=4, T=7, L=6, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"(a|b)*c", item_keys=[None] * 3,
                    candidates={None: _product("abc", 1, 5)}),
    "rows512_b32_k16": dict(B=32, k=16, T=7, L=5, C=97, eos=1, seed=100, chars="shipped", ci=False, patterns=r"[a-d0-3]+",
                            item_keys=[None] * 32, candidates={None: _product("abcd0123", 1, 4)}),
    "c256_identity": dict(B=2, k=5, T=7, L=5, C=256, eos=0, seed=100, chars="generic", ci=False,
                          patterns=lambda: "[" + "".join(_hi_chars()) + "]{2,}", item_keys=[None] * 2,
                          candidates={None: lambda: _product(_hi_chars(), 1, 4)()}),
    "t64": dict(B=2, k=3, T=64, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"a+b?|-\d", item_keys=[None] * 2,
                candidates={None: _product("ab-01234", 1, 4)}),
    "l64_a63": dict(B=2, k=2, T=7, L=64, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"a{63}", item_keys=[None] * 2,
                    candidates={None: lambda: iter(["a" * n for n in range(1, 64)])}, fc_scale=0.25, boost={"a": 12.0}),
    "two_segments": dict(B=5, k=3, T=7, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, patterns={"d": r"\d+", "w": r"[ab]+-?"},
                         item_keys=["d", "w", -1, 2, "w"],
                         candidates={"d": _product("01234", 1, 4), "w": _product("ab-", 1, 4)}),
}
# a language of at most k words, each shorter than L - 1: the finite hypotheses are exactly the language
EXHAUSTIVE = {
    "exhaustive_k4": dict(B=3, k=4, T=7, L=6, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"ab?|b1|-", item_keys=[None] * 3,
                          candidates={None: _product("ab1-", 1, 5)}),
}
CASES.update(EXHAUSTIVE)

_DATA = {}


def characters_of(case):
    ch = case["chars"]
    if ch == "shipped":
        return LC.shipped_characters()
    if ch == "generic":
        return LC.generic_characters(case["C"])
    return list(ch)


def patterns_of(case):
    p = case["patterns"]
    return p() if callable(p) else p


def language(regex, candidates, L, ci):
    """{w : re.fullmatch(regex, w), 1 <= |w| <= L - 1} among the candidates, in their order, without repeats"""
    rx = re.compile(regex, re.IGNORECASE if ci else 0)
    seen, out = set(), []
    for w in candidates:
        if 1 <= len(w) <= L - 1 and w not in seen and rx.fullmatch(w):
            seen.add(w)
            out.append(w)
    return out


def item_segments(d):
    """segment number of every item; an int item key is a segment number given as is (out of range on purpose)"""
    return [d["segment_names"].index(key) if key in d["segment_names"] else int(key) for key in d["item_keys"]]


def case_data(name):
    """-> dict: B k T L C eos, sd, x [B,T,D] float32 (CPU), characters, ci, patterns, segment_names, item_keys, words ({key:
    the enumerated language}), keys, roots, item_roots, f64 (the float64 replay of lexicon_beam_cases on the enumerated
    language).  Built once and shared; nothing in it is changed afterwards."""
    if name not in _DATA:
        c = CASES[name]
        B, k, T, L, C, eos = (c[n] for n in ("B", "k", "T", "L", "C", "eos"))
        chars = characters_of(c)
        assert len(chars) == C and len(c["item_keys"]) == B
        patterns = patterns_of(c)
        as_dict = patterns if isinstance(patterns, dict) else {None: patterns}
        names = list(as_dict)
        words = {key: language(rx, c["candidates"][key](), L, c["ci"]) for key, rx in as_dict.items()}
        sd = BC.decoder_sd(C, fc_scale=c.get("fc_scale", 1.0), eos=eos)
        for ch, add in c.get("boost", {}).items():
            sd[BC.Q + "fc.bias"][chars.index(ch)] += float(add)
        x = BC.rand_x(B, T, c["seed"])
        keys = LC.class_keys(chars, eos, c["ci"])
        roots, skipped, _ = LC.dict_tries({key: words[key] for key in names}, chars, L, eos, c["ci"])
        assert skipped == {"empty": 0, "too_long": 0, "no_class": 0}, skipped
        item_roots = [roots[names.index(key)] if key in names else None for key in c["item_keys"]]
        f64 = LC.replay(sd, x, k, C, L, eos, keys, item_roots)
        _DATA[name] = dict(B=B, k=k, T=T, L=L, C=C, eos=eos, sd=sd, x=x, characters=chars, ci=c["ci"], patterns=patterns,
                           segment_names=names, item_keys=c["item_keys"], words=words, keys=keys, roots=roots,
                           item_roots=item_roots, f64=f64)
    return _DATA[name]


def text_of(symbols, length, characters):
    """the string of one hypothesis: its symbols before the stop"""
    return "".join(characters[int(s)] for s in symbols[:max(int(length) - 1, 0)])


PROPERTY_REGEXES = [r"\d{2,4}", r"[A-Za-z]+\d?", r"(ab|cd)+e?", r"[^0-9a-z]{1,3}", r"x{30}"]      # the last: empty at L = 26


def rng_x(B, T, seed):
    return BC.rand_x(B, T, seed)

