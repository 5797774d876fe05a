"""CPU: the float64 restatement of the beam search (tests/beam_cases.py) against the reference's own function
(tests/golden/beam_search.npz), its back-tracking on hand-built decision tables, the path rows a hypothesis is handed to the
consumers of `pred_text_prob` as, and the cfg key that switches the search on."""
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -math.inf


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"] + list(opts))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_replay_reproduces_the_reference_golden(golden_dir, name):
    """widths 5, 3 and 1: best symbols identical, scores within 1e-4 (the tolerance tests/test_gpu_a_stages.py uses for
    this golden)"""
    g = np.load(os.path.join(golden_dir, "beam_search.npz"), allow_pickle=False)
    sd = BC.decoder_sd(97, 1234, float(g["fc_scale"]), float(g["bias0"]))
    x, width = torch.from_numpy(g[f"{name}:x"]), int(g[f"{name}:width"])
    r = BC.replay(sd, x, width, 97, 26, 0)
    assert r["symbols"][:, 0].tolist() == g[f"{name}:p"].tolist()
    d = float(np.abs(r["scores"][:, 0].numpy() - g[f"{name}:s"]).max())
    print(f"[beam] golden {name}: width {width}, max |dscore| {d:.3e}, selection gaps {r['sel_gap'].tolist()}, "
          f"final-score gaps {r['score_gap'].tolist()}")
    assert d < 1e-4
    assert r["symbols"].shape == (x.shape[0], width, 26) and (r["lengths"] >= 1).all() and (r["lengths"] <= 26).all()


def _tables(sc, pr, sy):
    f = lambda a, dt: torch.tensor(a, dtype=dt).unsqueeze(1)           # [L,k] -> [L,1,k]
    return f(sc, torch.float64), f(pr, torch.long), f(sy, torch.long)


def test_order_rule():
    assert BC.order(torch.tensor([NINF, 1.0, 1.0, NINF, 2.0], dtype=torch.float64)).tolist() == [4, 1, 2, 0, 3]


def test_backtrack_without_eos():
    sym, s, ln, st = BC.backtrack(*_tables([[-1, -2], [-2.5, -3], [-4, -3.5]], [[0, 0], [1, 0], [0, 0]], [[3, 4], [5, 6], [7, 8]]), 0)
    assert sym[0].tolist() == [[4, 5, 8], [4, 5, 7]] and s[0].tolist() == [-3.5, -4.0] and ln[0].tolist() == [3, 3]
    assert st[0, 0].tolist() == [-2.0, -2.5, -3.5] and st[0, 1].tolist() == [-2.0, -2.5, -4.0]


def test_backtrack_one_eos_midway():
    """slot 1 ends at step 1: it takes the worst result slot (k - 0 % k - 1 = 1) with the score it had there and wins the
    final re-sort; its symbol at step 2 is what the slot held before (the reference leaves it)"""
    sym, s, ln, st = BC.backtrack(*_tables([[-1, -2], [-2.5, -3], [-4, -4.5]], [[0, 0], [1, 0], [0, 0]], [[3, 4], [5, 0], [7, 8]]), 0)
    assert sym[0].tolist() == [[3, 0, 8], [4, 5, 7]] and s[0].tolist() == [-3.0, -4.0] and ln[0].tolist() == [2, 3]
    assert st[0, 0, :2].tolist() == [-1.0, -3.0]
    rows = BC.path_rows(sym[0, 0], st[0, 0], ln[0, 0], s[0, 0], 9)
    assert rows[0, 3] == math.exp(-1.0) and rows[1, 0] == math.exp(-2.0) and np.count_nonzero(rows) == 2


def test_backtrack_more_eos_than_slots_wraps_around():
    """three ended sequences, two slots: found % k wraps, the sequence that ended at step 2 is overwritten"""
    sym, s, ln, _ = BC.backtrack(*_tables([[-1, -1.5], [-2, -2.2], [-2.6, -5]], [[0, 0], [0, 0], [0, 0]], [[3, 0], [5, 0], [0, 8]]), 0)
    assert sym[0].tolist() == [[0, 5, 0], [3, 0, 0]] and s[0].tolist() == [-1.5, -2.2] and ln[0].tolist() == [1, 2]


def test_backtrack_eos_at_step_zero_then_live_beams():
    """the pattern of the golden's case `b`: a sequence that ended at step 0 outranks the live beams"""
    sym, s, ln, _ = BC.backtrack(*_tables([[-0.5, -1], [-2, -3]], [[0, 0], [1, 1]], [[0, 3], [4, 5]]), 0)
    assert sym[0].tolist() == [[0, 5], [3, 4]] and s[0].tolist() == [-0.5, -2.0] and ln[0].tolist() == [1, 2]


def test_backtrack_step_with_only_minus_inf_candidates():
    """width 1 after its <eos>: every candidate is -inf, the rule selects flat index 0 = <eos> again; going backwards the
    earliest end is the one that stays"""
    sym, s, ln, st = BC.backtrack(*_tables([[-1], [-1.5], [NINF]], [[0], [0], [0]], [[3], [0], [0]]), 0)
    assert sym[0].tolist() == [[3, 0, 0]] and s[0].tolist() == [-1.5] and ln[0].tolist() == [2]
    assert not BC.path_rows(sym[0, 0], st[0, 0], 3, NINF, 5).any()               # a -inf hypothesis: all-zero rows


def test_replay_selects_by_index_among_minus_inf():
    """k == C == 2 with equal logits: step 0 has exactly k finite candidates, a tie that the flat index decides; slot 0 ends
    there, so from step 1 on the two finite candidates are those of slot 1.  Width 1 whose only beam has ended: every
    candidate is -inf and flat index 0 is taken."""
    def step(state, y):
        return torch.zeros((state.shape[0], 2), dtype=torch.float64), state
    r = BC.replay_with(step, torch.zeros((2, 1), dtype=torch.float64), 1, 2, 2, 3, eos=0)
    sc, pr, sy = r["tables"]
    assert sy[:, 0].tolist() == [[0, 1], [0, 1], [0, 1]] and pr[:, 0].tolist() == [[0, 0], [1, 1], [1, 1]]
    assert sc[:, 0].tolist() == [[i * math.log(0.5)] * 2 for i in (1, 2, 3)]
    assert r["symbols"][0].tolist() == [[0, 1, 0], [1, 0, 0]] and r["lengths"][0].tolist() == [1, 2]
    r = BC.replay_with(step, torch.zeros((1, 1), dtype=torch.float64), 1, 1, 2, 3, eos=0)
    sc, pr, sy = r["tables"]
    assert sy[:, 0, 0].tolist() == [0, 0, 0] and sc[:, 0, 0].tolist() == [math.log(0.5), NINF, NINF]
    assert r["scores"][0].tolist() == [math.log(0.5)] and r["lengths"][0].tolist() == [1]


def test_path_rows_feed_the_text_decoder():
    """one non-zero entry per row below the length and none after, their product is exp(score), and the text decoder reads
    the same word from arg-max / max of the rows as from the symbols"""
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    enc = TextEncoder(_cfg())
    stop = enc.character.index("[s]")
    sd = BC.decoder_sd(97, 1234, 6.0, 2.0, eos=stop)
    r = BC.replay(sd, BC.rand_x(4, 32, 7), 3, 97, 26, stop)
    ended = 0
    for b in range(4):
        sym, n, score = r["symbols"][b, 0], int(r["lengths"][b, 0]), float(r["scores"][b, 0])
        rows = BC.path_rows(sym, r["step_scores"][b, 0], n, score, 97)
        assert (np.count_nonzero(rows, axis=1) == np.array([1] * n + [0] * (26 - n))).all()
        assert rows[np.arange(n), sym[:n].numpy()].all()
        assert abs(float(np.prod(rows.max(1)[:n])) - math.exp(score)) <= 1e-12 * math.exp(score)
        via_rows = enc.decode_attention(rows.argmax(1)[None], rows.max(1)[None].copy())[0]
        direct = enc.decode_attention(sym.numpy()[None])[0]
        assert via_rows["text"] == direct["text"]
        assert abs(float(via_rows["score"]) - math.exp(score)) <= 1e-12 * math.exp(score)
        ended += n < 26
    assert ended, "no hypothesis ended inside the 26 steps: the case does not exercise the zero rows"


def test_beam_width_key_defaults_to_greedy_and_reaches_the_head():
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    assert get_glass_cfg().MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH == 0 and _cfg().MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH == 0
    # (that the reference's own YAMLs still load is tests/test_host.py::test_config_accepts_reference_yamls_verbatim)
    assert RecognizerRCNNHeadV3(_cfg(), ShapeSpec(channels=256)).beam_width == 0
    assert RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3]), ShapeSpec(channels=256)).beam_width == 3
    with pytest.raises(ValueError):
        RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 17]), ShapeSpec(channels=256))


def test_beam_search_entries_are_declared_and_have_no_cpu_fallback():
    from glass_amd import _lib
    from glass_amd.ops import native as K
    hdr = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("glass_beam_search_workspace_bytes", "glass_beam_search"):
        assert name in _lib.EXPORTS and name + "(" in hdr, name
    assert _lib.ABI_VERSION == 8                                          # additive change
    x = torch.zeros((1, 4, 256))
    with pytest.raises(_lib.GlassLibraryError):
        K.beam_search(x, x, {}, 2, 97, 26, 0)


# ------------------------------------------------------------------ the host side every beam search shares
@pytest.mark.parametrize("B,k,L,beam,nodes,weighted", [(3, 5, 26, 66120, 67680, 70800), (1, 16, 64, 77824, 81920, 90112),
                                                       (1, 1, 1, 4108, 4112, 4120), (0, 5, 26, 0, 0, 0)])
def test_workspace_bytes_of_every_beam_search(B, k, L, beam, nodes, weighted):
    """hsel | hraw | inp (2x) | sc | pr | sy | nd | wa | fu: four state blocks of B*k*D*4 bytes and three tables of B*L*k*4
    bytes, one more table for a node-constrained search, three more for a weighted one; nothing for an empty batch.  The
    expected sizes are that formula worked out by hand."""
    from glass_amd import _lib
    _lib.build_library()
    lib = _lib.lib()
    for name, want in (("", beam), ("_lexicon", nodes), ("_dfa", nodes), ("_merged_dfa", nodes), ("_wdfa", weighted),
                       ("_merged_wdfa", weighted)):
        assert getattr(lib, f"glass_beam_search{name}_workspace_bytes")(B, k, 32, 256, 97, L) == want, name


_PTR = 4096                 # never dereferenced: every refusal comes before the first runtime call


def _refusal_call(lib, entry, B=2, k=3, N=4, scale=1.0, n=11, out=_PTR, arr=_PTR, trans=_PTR, ws=1 << 40):
    """one call of `entry` with T=8, D=256, C=13, max_len=5, S=1, F=11: `out` = its last mandatory output, `arr` = one of its
    constraint's arrays (forced decoding: the targets), `trans` = the weighted table, n = n_group_cls"""
    p = _PTR
    head = [p, p, p, B, k, 8, 256, 13, 5, 1]
    tail = [None, p, ws, None]
    fn = getattr(lib, entry)
    if entry == "glass_beam_search":
        return fn(*head, p, p, out, *tail)
    if entry == "glass_forced_decode":
        return fn(*head, arr, None, p, p, out, None, *tail)
    if entry == "glass_beam_search_lexicon":
        return fn(*head, p, p, arr, p, p, N, 1, 11, p, p, p, p, out, *tail)
    groups = [p, p, n] if "merged" in entry else []
    if entry.endswith("_wdfa"):
        return fn(*head, trans, arr, p, p, p, p, N, 1, 11, p, scale, *groups, p, p, p, p, out, *tail)
    return fn(*head, p, arr, p, p, N, 1, 11, p, *groups, p, p, p, out, *tail)


_INF = float("inf")
_LIMITS = ": needs D=256, 1<=T<=64, 1<=C<=256, 1<=k<=16, k<=C, 1<=max_len<=64, B>=0 (got B=2 k=17 T=8 D=256 C=13 max_len=5)"
_AUTOMATON = ": needs 1<=N<2^24, S>=1, 1<=F<=256 (got N=0 S=1 F=11)"
# (entry point, two faults from adjacent stages of the check order, the message of the first - None: B == 0 returns 0)
_FIRST_REFUSALS = [
    ("glass_beam_search", dict(k=17, out=None), _LIMITS),
    ("glass_beam_search", dict(k=17, B=0), ": needs D=256, 1<=T<=64, 1<=C<=256, 1<=k<=16, k<=C, 1<=max_len<=64, B>=0 (got B=0 k=17 T=8 D=256 C=13 max_len=5)"),
    ("glass_beam_search", dict(B=0, out=None), None),
    ("glass_beam_search", dict(out=None, ws=16), ": null pointer"),
    ("glass_forced_decode", dict(k=17, out=None), ": needs D=256, 1<=T<=64, 1<=C<=256, 1<=n<=16, 1<=max_len<=64, B>=0 (got B=2 n=17 T=8 D=256 C=13 max_len=5)"),
    ("glass_forced_decode", dict(k=17, B=0), ": needs D=256, 1<=T<=64, 1<=C<=256, 1<=n<=16, 1<=max_len<=64, B>=0 (got B=0 n=17 T=8 D=256 C=13 max_len=5)"),
    ("glass_forced_decode", dict(B=0, out=None), None),
    ("glass_forced_decode", dict(out=None, ws=16), ": null pointer"),
    ("glass_forced_decode", dict(arr=None, ws=16), ": null pointer"),
    ("glass_beam_search", dict(ws=16), ": workspace too small (16 < 24936 bytes)"),
    ("glass_forced_decode", dict(ws=16), ": workspace too small (16 < 24624 bytes)"),
    ("glass_beam_search_lexicon", dict(k=17, N=0), _LIMITS),
    ("glass_beam_search_lexicon", dict(N=0, B=0), ": needs N>=1, S>=1, 1<=F<=256 (got N=0 S=1 F=11)"),
    ("glass_beam_search_lexicon", dict(B=0, out=None), None),
    ("glass_beam_search_lexicon", dict(out=None, arr=None), ": null pointer"),
    ("glass_beam_search_lexicon", dict(arr=None, ws=16), ": null trie array"),
    ("glass_beam_search_lexicon", dict(ws=16), ": workspace too small (16 < 25056 bytes)"),
    ("glass_beam_search_dfa", dict(k=17, N=0), _LIMITS),
    ("glass_beam_search_dfa", dict(N=0, B=0), _AUTOMATON),
    ("glass_beam_search_dfa", dict(B=0, out=None), None),
    ("glass_beam_search_dfa", dict(out=None, arr=None), ": null pointer"),
    ("glass_beam_search_dfa", dict(arr=None, ws=16), ": null automaton array"),
    ("glass_beam_search_dfa", dict(ws=16), ": workspace too small (16 < 25056 bytes)"),
    ("glass_beam_search_merged_dfa", dict(k=17, N=0), _LIMITS),
    ("glass_beam_search_merged_dfa", dict(N=0, B=0), _AUTOMATON),
    ("glass_beam_search_merged_dfa", dict(N=0, n=0), _AUTOMATON),
    ("glass_beam_search_merged_dfa", dict(n=0, B=0), ": needs 1<=n_group_cls<=C (got n_group_cls=0 C=13)"),
    ("glass_beam_search_merged_dfa", dict(B=0, out=None), None),
    ("glass_beam_search_merged_dfa", dict(out=None, arr=None), ": null pointer"),
    ("glass_beam_search_merged_dfa", dict(arr=None, ws=16), ": null automaton array"),
    ("glass_beam_search_merged_dfa", dict(ws=16), ": workspace too small (16 < 25056 bytes)"),
    ("glass_beam_search_wdfa", dict(k=17, N=0), _LIMITS),
    ("glass_beam_search_wdfa", dict(N=0, B=0), _AUTOMATON),
    ("glass_beam_search_wdfa", dict(N=0, scale=_INF), _AUTOMATON),
    ("glass_beam_search_wdfa", dict(scale=_INF, B=0), ": weight_scale must be finite (got inf)"),
    ("glass_beam_search_wdfa", dict(B=0, out=None), None),
    ("glass_beam_search_wdfa", dict(out=None, arr=None), ": null pointer"),
    ("glass_beam_search_wdfa", dict(arr=None, ws=16), ": null automaton array"),
    ("glass_beam_search_wdfa", dict(arr=None, trans=4100), ": null automaton array"),
    ("glass_beam_search_wdfa", dict(trans=4100, ws=16), ": trans is not 8-byte aligned"),
    ("glass_beam_search_wdfa", dict(ws=16), ": workspace too small (16 < 25296 bytes)"),
    ("glass_beam_search_merged_wdfa", dict(k=17, N=0), _LIMITS),
    ("glass_beam_search_merged_wdfa", dict(N=0, B=0), _AUTOMATON),
    ("glass_beam_search_merged_wdfa", dict(N=0, scale=_INF), _AUTOMATON),
    ("glass_beam_search_merged_wdfa", dict(scale=_INF, B=0), ": weight_scale must be finite (got inf)"),
    ("glass_beam_search_merged_wdfa", dict(N=0, n=0), _AUTOMATON),
    ("glass_beam_search_merged_wdfa", dict(n=0, B=0), ": needs 1<=n_group_cls<=C (got n_group_cls=0 C=13)"),
    ("glass_beam_search_merged_wdfa", dict(scale=_INF, n=0), ": weight_scale must be finite (got inf)"),
    ("glass_beam_search_merged_wdfa", dict(B=0, out=None), None),
    ("glass_beam_search_merged_wdfa", dict(out=None, arr=None), ": null pointer"),
    ("glass_beam_search_merged_wdfa", dict(arr=None, ws=16), ": null automaton array"),
    ("glass_beam_search_merged_wdfa", dict(arr=None, trans=4100), ": null automaton array"),
    ("glass_beam_search_merged_wdfa", dict(trans=4100, ws=16), ": trans is not 8-byte aligned"),
    ("glass_beam_search_merged_wdfa", dict(ws=16), ": workspace too small (16 < 25296 bytes)"),
]


@pytest.mark.parametrize("entry,faults,message", _FIRST_REFUSALS)
def test_first_refusal_of_every_search(entry, faults, message):
    """the order of the host-side checks: the search's limits, the automaton's, weight_scale, the groups', B == 0, null
    pointers, null arrays and alignment, the workspace.  Every call carries two faults; the earlier stage answers."""
    from glass_amd import _lib
    _lib.build_library()
    lib = _lib.lib()
    rc = _refusal_call(lib, entry, **faults)
    if message is None:
        assert rc == 0
        return
    assert rc < 0
    assert lib.glass_last_error().decode() == entry + message
