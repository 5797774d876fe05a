"""CPU: the exact-tie cases of the decoder searches (tests/search_tie_cases.py) are what they claim to be - properties of the
inputs and the stated rule alone, checked without a device: every candidate pair a decision rests on is exactly equal in
float64 AND in float32, or more than MARGIN apart; every case has a tie that DECIDES a selection; the restatement agrees with
the existing float64 replays; and a rule that took the higher index on a tie would decide every case differently."""
import math

import pytest
import torch

import beam_cases as BC
import search_tie_cases as S


def _higher_index_first(v):
    """beam_cases.order with the tie-break the wrong way round: value descending, then index DESCENDING, -inf last"""
    return len(v) - 1 - torch.sort(-v.flip(0), stable=True).indices


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_meets_the_condition_and_has_a_decisive_tie(name):
    """`case_data` raises where a pair is a near-tie or float64 and float32 decide differently; the counts are printed"""
    d = S.case_data(name)
    n = d["count"]
    print(f"[ties] {name}: {n['ties']} exact ties between neighbouring candidates, {n['decisive']} of them decisive (the k-th "
          f"selected = the best not selected), {n['decisive_ninf']} cuts between two -inf candidates, {n['final_ties']} ties "
          f"between neighbouring final scores")
    if "only" in S.CASES[name]:
        assert n["decisive_ninf"] >= 1 and n["ties"] == 0          # the all-ended case: every tie is between -inf candidates
    else:
        assert n["decisive"] >= 1, "no tie decides a selection: replace the case"
        assert n["ties"] > n["decisive"]


@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_is_the_existing_replay(name):
    """in float64 the restatement and the replay of the neighbouring case module give the same hypotheses and scores"""
    d = S.case_data(name)
    f64, r64 = d["f64"], d["r64"]
    assert torch.equal(f64["symbols"], r64["symbols"]) and torch.equal(f64["lengths"], r64["lengths"])
    if r64["words"] is not None:
        assert torch.equal(f64["words"], r64["words"])
    for mine, theirs in ((r64["scores"], f64["scores"]), (r64["model_scores"], S.model_scores_of(f64))):
        assert torch.equal(torch.isneginf(mine), torch.isneginf(theirs))
        fin = torch.isfinite(theirs)
        assert float((mine[fin] - theirs[fin]).abs().max() if fin.any() else 0.0) < 1e-12
    if d["search"] == "plain":
        assert torch.equal(f64["tables"][1], r64["pr"]) and torch.equal(f64["tables"][2], r64["sy"])
        assert float(f64["sel_gap"].min()) == 0.0 or "only" in S.CASES[name]


def test_the_rule_predicts_the_flat_cases():
    """hand-derived from the rule, not from any replay"""
    d = S.case_data("flat_c256_k3_four_waves")                    # never ends: beam 0's classes 5, 70, 130 at every step
    assert d["r64"]["sy"][:, 0].tolist() == [[5, 70, 130]] * 4 and d["r64"]["pr"][1:, 0].tolist() == [[0, 0, 0]] * 3
    assert d["f64"]["symbols"][0].tolist() == [[5, 5, 5, 5], [5, 5, 5, 70], [5, 5, 5, 130]]
    d = S.case_data("flat_c97_k5_two_levels_l2")                  # step 1: four lA + lA, then beam 0's lA + lB before lB + lA
    assert d["r64"]["sy"][0, 0].tolist() == [10, 80, 5, 30, 64]
    assert (d["r64"]["pr"][1, 0] * 97 + d["r64"]["sy"][1, 0]).tolist() == [10, 80, 97 + 10, 97 + 80, 5]
    d = S.case_data("flat_c13_k5_eos_low")                        # all final scores equal: the slots keep their order
    assert d["f64"]["symbols"][1].tolist() == [[1] * 5 + [c] for c in (1, 4, 6, 8, 10)]
    assert len(set(d["f64"]["scores"][1].tolist())) == 1
    d = S.case_data("flat_c13_k3_all_ended")
    assert d["f64"]["scores"][0].tolist() == [0.0, -math.inf, -math.inf] and d["f64"]["lengths"][0].tolist() == [1, 2, 3]
    d = S.case_data("flat_merged_k3")                             # the groups a/A and b/B tie: representatives 2 and 3, beam 0 first
    assert (d["r64"]["pr"][1, 0] * 13 + d["r64"]["sy"][1, 0]).tolist() == [2, 3, 13 + 2]


def test_twin_seeds_are_the_first_that_qualify():
    for name, c in S.CASES.items():
        if c["decoder"] == "twin":
            assert S.find_seed(name) == c["seed"], name


def test_a_near_tie_is_rejected():
    """two levels 1e-5 apart: neither equal nor MARGIN apart"""
    c = dict(S.CASES["flat_c13_k3_eos_mid"])
    sd = S.flat_sd(c)
    sd[BC.Q + "fc.bias"][6] -= 1e-5
    d = S.case_inputs("flat_c13_k3_eos_mid")
    d["step"] = S.flat_step(sd)
    with pytest.raises(AssertionError, match="near-tie"):
        S.check_inputs(d)


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_higher_index_on_a_tie_decides_differently(name, monkeypatch):
    """the mutation a kernel could hide: with the tie-break reversed (in the selection and in both final sorts) the float32
    restatement reaches other decision tables on every case - each case can tell the two rules apart"""
    d = S.case_data(name)
    monkeypatch.setattr(BC, "order", _higher_index_first)
    wrong = S._restate(d, torch.float32)
    assert not (torch.equal(wrong["pr"], d["r64"]["pr"]) and torch.equal(wrong["sy"], d["r64"]["sy"])), name
    assert not torch.equal(wrong["symbols"], d["r64"]["symbols"]), name
