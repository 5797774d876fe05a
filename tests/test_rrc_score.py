"""CPU: the host side of the RRC scorer (glass_amd/evaluation/rrc_score.py: parsing, care rules, transcription match,
tallies from match lists), the exported symbols, and the exact checker of tests/rrc_cases.py on known answers."""
import io
import zipfile
from fractions import Fraction as F

import pytest

import rrc_cases as C


def _zip(entries):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        for name, data in entries.items():
            z.writestr(name, data)
    return buf.getvalue()


def test_parsers_both_line_formats():
    from glass_amd.evaluation import rrc_score as R
    assert R.parse_gt_line("377,117,463,117,465,130,378,130,Genaxis Theatre", "icdar") == \
        ([377, 117, 463, 117, 465, 130, 378, 130], "Genaxis Theatre")
    assert R.parse_gt_line(" 1 , 2,3,4, -5,6,7,8, keeps blanks ", "icdar") == ([1, 2, 3, 4, -5, 6, 7, 8], " keeps blanks ")
    assert R.parse_gt_line("1,2,3,4,5,6,7,8,###", "icdar")[1] == "###"
    assert R.parse_gt_line('1,2,3,4,5,6,7,8,"say \\"hi\\" \\\\ bye"', "icdar")[1] == 'say "hi" \\ bye'
    assert R.parse_gt_line("1,2,3,4,5,6,7,8,a,b,####c", "icdar")[1] == "a,b,####c"
    assert R.parse_gt_line("  10,20,30.0,20,30,40,20,45,10,40,####  curved text \r", "totaltext") == \
        ([10, 20, 30, 20, 30, 40, 20, 45, 10, 40], "curved text")
    assert R.parse_gt_line('1,1,5,1,5,5,####"q\\"x"', "totaltext")[1] == 'q"x'
    assert R.parse_gt_line("1,1,5,1,5,5,####a,####b", "totaltext")[1] == "a"          # only the first piece is the word
    for bad, fmt in (("1,2,3,4,5,6,7,text", "icdar"), ("1.5,2,3,4,5,6,7,8,t", "icdar"), ("1,2,3,####t", "totaltext"),
                     ("1,2,3,4,5,6", "totaltext"), ("1,2,3.5,4,5,6,####t", "totaltext"), ("1,2,x,4,5,6,####t", "totaltext"),
                     ("1,2,3,4,5,1048577,####t", "totaltext"), ("1,2,inf,4,5,6,####t", "totaltext")):
        with pytest.raises(ValueError):
            R.parse_gt_line(bad, fmt)
    assert R.parse_gt_line("1,2,3,4,-1048576,1048576,####t", "totaltext")[0][-2:] == [-1048576, 1048576]
    # detections: clockwise as normalize_detection_line emits (negative shoelace), simple, non-degenerate
    assert R.parse_detection_line("0,10,10,10,10,0,0,0,####  Word ") == ([0, 10, 10, 10, 10, 0, 0, 0], "Word")
    for bad in ("0,0,10,0,10,10,0,10,####ccw", "0,0,10,0,####two", "0,0,5,0,10,0,####flat", "0,20,10,0,10,10,0,0,####bowtie",
                "0,10,10,10,10,0,0,0", "0,10,10,10,10,0.5,0,0,####x"):
        with pytest.raises(ValueError):
            R.parse_detection_line(bad)
    assert R.parse_detection_line("0,20,10,0,10,10,0,0,####bowtie", validate=False)[1] == "bowtie"   # the quadratic test is optional
    from glass_amd.evaluation import normalize_detection_line
    for line in ("3,4,50,6,48,30,2,28,####ok", "0,0,0,10,10,10,10,0,####ok"):
        n = normalize_detection_line(line)
        assert R.parse_detection_line(n)[1] == "ok"


def test_zip_loading_bom_crlf_off_and_names():
    from glass_amd.evaluation import rrc_score as R
    gt = _zip({"gt_img_2.txt": b"\xef\xbb\xbf1,2,3,4,5,6,7,8,caf\xc3\xa9\r\n\r\n9,9,19,9,19,19,9,19,###\n", "gt_img_10.txt": b"",
               "readme.md": b"skipped", "gt_img_3.txt": b"1,2,3,4,5,6,7,8,bad\xff\n"})
    out = R.load_gt_zip(gt, "icdar")
    assert list(out) == ["2", "10", "3"]                         # archive order, keys as written
    assert out["2"] == ([[1, 2, 3, 4, 5, 6, 7, 8], [9, 9, 19, 9, 19, 19, 9, 19]], ["café", "###"])   # BOM gone, CR removed
    assert out["10"] == ([], []) and out["3"][1] == ["bad�"]
    tt = _zip({"0000007.txt": b"1,1,9,1,9,9,5,12,1,9,####word\n", "gt_img_1.txt": b"not matched by ([0-9]+).txt"})
    assert R.load_gt_zip(tt, "totaltext") == {"0000007": ([[1, 1, 9, 1, 9, 9, 5, 12, 1, 9]], ["word"])}
    assert R.gt_line_format("/data/totaltext/gt.zip") == "totaltext" and R.gt_line_format("/d/textocr_gt.zip") == "totaltext"
    assert R.gt_line_format("/data/ic15/gt.zip") == "icdar" and R.gt_line_format(b"PK") == "icdar"
    with pytest.raises(ValueError):
        R.load_gt_zip(_zip({"gt_img_1.txt": b"1,2,3,4,5,6,7,oops\n"}), "icdar")
    sub = R.load_submission(_zip({"7.txt": b"0,10,10,10,10,0,0,0,####a\r\n\n"}))
    assert sub == {"7": ["0,10,10,10,10,0,0,0,####a"]}
    assert R.load_submission({"0000007.txt": ["l1\n", "", "l2"]}) == {"0000007": ["l1", "l2"]}
    with pytest.raises(ValueError):
        R.load_submission(_zip({"notes.md": b""}))               # every entry of a submission must be a result file
    with pytest.raises(ValueError):
        R.load_submission(b"not a zip")


def test_include_in_dictionary_table():
    from glass_amd.evaluation import include_in_dictionary, include_in_dictionary_transcription
    table = {"hello": True, "John's": True, "JOHN'S": True, "it's": False, "ab": False, "abc": True, "-dash-": True, "a-b": True,
             "--ab--": False, "two words": False, "don't": False, "x×y": False, "a÷bc": False, "exit!": True, "(note)": True,
             "café": True, "Ünï": True, "Ǆab": True, "Άβγ": True, "АБВ": False,
             "abc1": False, "42nd": False, "e.g.": False, "": False, "!!!": False, "a·b·c": False, "abc#": False,
             "ǀab": False, "ʀbc": False}
    for word, want in table.items():
        assert include_in_dictionary(word) is want, word
    forms = {"John's": "John", "-dash-": "dash", "exit!": "exit", "(note)": "note", "a.b": "a b", "'s": "", "it's": "it"}
    for word, want in forms.items():
        assert include_in_dictionary_transcription(word) == want, word


def test_transcription_match_and_care_rules():
    from glass_amd.evaluation import rrc_score as R
    table = [("HELLO", "HELLO", True), ("HELLO!", "HELLO", True), ("(HELLO", "HELLO", True), ("(HELLO)", "HELLO", True),
             ("(HELLO)", "HELLO)", True), ("((HELLO", "HELLO", False), ("HELLO", "HELLO!", False), ("HEL.LO", "HELLO", False),
             ("", "", True), ("", "X", False), ("!", "", True), ("!", "!", True), ("!?", "", True), ("A", "", False),
             ("'TIS", "TIS", True), ("A·", "A", True)]
    for gt, det, want in table:
        assert R.transcription_match(gt, det) is want, (gt, det)
    assert R.pair_correct("Hello!", "hello", False) and not R.pair_correct("Hello!", "hello", True)
    assert R.pair_correct("a####b", "AB", True) and not R.pair_correct("", "x", False)
    trans, e2e, det = R.ground_truth_care(["###", "John's", "ab", "two words", "exit!"], True)
    assert (trans, e2e, det) == (["###", "John", "ab", "two words", "exit"], [True, False, True, True, False],
                                 [True, False, False, False, False])
    trans, e2e, det = R.ground_truth_care(["###", "John's", "ab"], False)
    assert (trans, e2e, det) == (["###", "John's", "ab"], [True, False, False], [True, False, False])


def _sample(texts, word_spotting=False):
    from glass_amd.evaluation import rrc_score as R
    trans, e2e, det = R.ground_truth_care(texts, word_spotting)
    return R.GroundTruthSample([[0, 0, 1, 0, 1, 1, 0, 1]] * len(texts), list(texts), trans, e2e, det)


def test_tallies_from_match_lists():
    from glass_amd.evaluation import rrc_score as R
    box = [0, 1, 1, 1, 1, 0, 0, 0]
    # two care GT, one don't-care; three detections: one right, one wrong word, one on the don't-care GT
    s, c = R.tally_sample(_sample(["cat", "dog!", "###"]), [box] * 3, ["CAT", "bird", "x"], [0, 1, -1], [0, 1, -1], [0, 0, 1], [0, 0, 1],
                          [[1.0, 0.0, 0.0]] * 3, False)
    assert c == R.SampleCounts(1, 2, 2, 2, 2, 2)
    assert (s["precision"], s["recall"], s["hmean"]) == (0.5, 0.5, 0.5)
    assert s["gtDontCare"] == [2] and s["detDontCare"] == [2] and s["gtTrans"] == ["cat", "dog!", "###"]
    assert s["detTrans"] == ["CAT", "bird", "x"] and s["iouMat"] == [[1.0, 0.0, 0.0]] * 3
    assert s["gtPolPoints"][0] == [0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0] and s["detPolPoints"] == [[float(v) for v in box]] * 3
    # no care GT: recall 1, precision 0 with care detections, 1 without
    s1, c1 = R.tally_sample(_sample(["###"]), [box], ["a"], [-1], [-1], [0], [0], [[0.0]], False)
    assert (s1["precision"], s1["recall"], s1["hmean"]) == (0.0, 1.0, 0.0) and c1 == R.SampleCounts(0, 0, 1, 0, 0, 1)
    s2, c2 = R.tally_sample(_sample(["###"]), [box], ["a"], [-1], [-1], [1], [1], [[0.9]], False)
    assert (s2["precision"], s2["recall"], s2["hmean"]) == (1.0, 1.0, 1.0) and c2 == R.SampleCounts(0, 0, 0, 0, 0, 0)
    # image missing from the submission / no detections: precision is the integer 0 the reference leaves there
    s3, c3 = R.tally_sample(_sample(["cat", "dog"]), [], [], [-1, -1], [-1, -1], [], [], None, False)
    assert (s3["precision"], s3["recall"], s3["hmean"]) == (0, 0.0, 0) and str(s3["precision"]) == "0" and s3["iouMat"] == []
    assert c3 == R.SampleCounts(0, 2, 0, 0, 2, 0)
    # empty image and empty submission
    s4, c4 = R.tally_sample(_sample([]), [], [], [], [], [], [], None, False)
    assert (s4["precision"], s4["recall"], s4["hmean"]) == (1.0, 1.0, 1.0) and c4 == R.SampleCounts(0, 0, 0, 0, 0, 0)
    # word spotting: 'ab' is don't-care end-to-end only; equality decides
    s5, c5 = R.tally_sample(_sample(["John's", "ab"], True), [box] * 2, ["john", "ab"], [0, -1], [0, 1], [0, 1], [0, 0], None, True)
    assert c5 == R.SampleCounts(1, 1, 1, 2, 2, 2) and s5["gtTrans"] == ["John", "ab"] and s5["gtDontCare"] == [1]
    # more than 100 detections: no iouMat
    s6, _ = R.tally_sample(_sample(["cat"]), [box] * 101, ["x"] * 101, [-1], [-1], [0] * 101, [0] * 101, [[0.0] * 101], False)
    assert s6["iouMat"] == []
    e2e, det = R.method_strings([c, c1, c2, c3, c4])
    assert e2e == "E2E_RESULTS: precision: 0.3333333333333333, recall: 0.25, hmean: 0.28571428571428575"
    assert det == "DETECTION_ONLY_RESULTS: precision: 0.6666666666666666, recall: 0.5, hmean: 0.5714285714285715"
    assert R.method_strings([]) == ("E2E_RESULTS: precision: 0, recall: 0, hmean: 0", "DETECTION_ONLY_RESULTS: precision: 0, recall: 0, hmean: 0")
    assert R.method_strings([c3]) == ("E2E_RESULTS: precision: 0, recall: 0.0, hmean: 0", "DETECTION_ONLY_RESULTS: precision: 0, recall: 0.0, hmean: 0")
    assert R.method_strings([R.SampleCounts(3, 3, 3, 3, 3, 3)])[0] == "E2E_RESULTS: precision: 1.0, recall: 1.0, hmean: 1.0"
    assert R.parse_method_string(e2e) == ("E2E_RESULTS", {"precision": 0.3333333333333333, "recall": 0.25, "hmean": 0.28571428571428575})
    assert R.iou_matrix(__import__("numpy").array([[0.0, 50.0]]), __import__("numpy").array([0.0]),
                        __import__("numpy").array([0.0, 100.0])).tolist() == [[0.0, 1.0]]


def test_new_symbols_exported_and_abi_unchanged():
    from glass_amd import _lib
    for name in ("glass_rrc_pair_areas_workspace_bytes", "glass_rrc_pair_areas", "glass_rrc_match_workspace_bytes", "glass_rrc_match"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    from glass_amd.evaluation import RRCScorer, TextResultWriter        # noqa: F401
    assert hasattr(TextResultWriter, "evaluate")
    import torch
    from glass_amd.ops import native as K
    with pytest.raises(_lib.GlassLibraryError):                          # no CPU fallback
        K.rrc_pair_areas(torch.zeros((4, 2), dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
                         torch.tensor([1, 1], dtype=torch.int32), torch.tensor([0, 0]), 0)
    with pytest.raises(_lib.GlassLibraryError):
        RRCScorer({"1": ([[0, 0, 1, 0, 1, 1]], ["a"])}, False, "cpu")


def test_exact_checker_known_answers():
    rect = lambda x, y, w, h: [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    L = [(0, 0), (10, 0), (10, 4), (4, 4), (4, 10), (0, 10)]
    concave = [(0, 0), (10, 0), (10, 10), (5, 4), (0, 10)]                # a notch from the top down to (5, 4)
    tri = [(0, 10), (10, 10), (5, 2)]                                     # apex inside the notch's shadow
    known = [(rect(0, 0, 10, 10), rect(1, 1, 10, 10), F(81)), (L, rect(2, 2, 6, 6), F(20)), (rect(0, 0, 10, 10), rect(20, 0, 3, 3), F(0)),
             (rect(0, 0, 100, 100), rect(40, 40, 5, 5), F(25)), (rect(0, 0, 10, 10), rect(10, 0, 10, 10), F(0)),
             (rect(0, 0, 10, 10), rect(0, 0, 10, 4), F(40)), ([(0, 0), (10, 0), (0, 10)], [(10, 10), (0, 10), (10, 0)], F(0)),
             ([(0, 0), (2, 0), (0, 2)], [(0, 0), (2, 0), (2, 2)], F(1)), ([(0, 0), (3, 0), (0, 3)], [(0, 0), (3, 0), (3, 3)], F(9, 4))]
    for A, B, want in known:
        for P, Q in ((A, B), (B, A), (A[::-1], B), (A[2:] + A[:2], B[::-1])):
            assert C.exact_intersection(P, Q) == want, (P, Q)
    # concave ring against a triangle: inclusion-exclusion with the notch (itself a triangle) as the third set
    notch = [(0, 10), (10, 10), (5, 4)]
    square = rect(0, 0, 10, 10)
    assert C.exact_area(concave) == 70 and C.exact_area(notch) == 30
    assert C.exact_intersection(concave, tri) == C.exact_intersection(square, tri) - C.exact_intersection(notch, tri)
    assert C.exact_intersection(notch, tri) == 30 and C.exact_intersection(concave, tri) == 10
    assert C.exact_intersection(concave, concave) == 70


def test_exact_protocol_on_the_tie_case():
    gt, sub, want = C.tie_case()
    for ws in (False, True):
        res = C.check_score(gt, sub, ws)
        for key, w in want.items():
            assert tuple(res["per_sample"][key]["decisions"]) == w, key
    res = C.check_score(gt, sub, False)
    assert res["per_sample"]["1"]["iouMat"] == [[F(1, 2)]] and res["per_sample"]["6"]["iouMat"] == [[F(0)]]
    assert res["e2e_method"] == "E2E_RESULTS: precision: 0.3333333333333333, recall: 0.4, hmean: 0.3636363636363636"   # 2 of 6 / 2 of 5
    with pytest.raises(ValueError):
        C.check_score(gt, {"9": []}, False)


def test_decisions_golden_is_what_the_checker_derives_on_a_sample():
    """The recorded answers of the large case (tests/golden/rrc_decisions.json): the case regenerates to the recorded
    digest from the recorded redraws, and on a sample of images the exact checker re-derives the decisions and finds no
    pair inside the decision bands."""
    gold = C.load_decisions_golden()
    gt, sub, planted, _ = C.decisions_case(redraws=gold["redraws"])
    assert len(gt) >= 200 and C.case_digest(gt, sub) == gold["digest"] and planted == gold["planted"]
    keys = planted[:6] + [k for k in gt if k not in planted][::9]
    sgt = {k: gt[k] for k in keys}
    ssub = {k: sub[k] for k in keys if k in sub}
    for ws, name in ((False, "e2e"), (True, "word_spotting")):
        res = C.recorded(C.check_score(sgt, ssub, ws))
        for k in keys:
            assert res["per_sample"][k] == gold[name]["per_sample"][k], (name, k)
    n = 0
    for k in keys:
        if k in planted or k not in sub:
            continue
        from glass_amd.evaluation.rrc_score import parse_detection_line
        for line in sub[k]:
            P = C.ring(parse_detection_line(line)[0])
            for flat in gt[k][0]:
                Gr = C.ring(flat)
                i, ag, ad, b = C.exact_intersection(Gr, P), C.exact_area(Gr), C.exact_area(P), C.inter_bound(Gr, P)
                assert abs(2 * i - (ag + ad - i)) > C.iou_band(b, ag + ad - i) and abs(2 * i - ad) > C.dontcare_band(b, ad)
                n += 1
    assert n > 100
    # the case has what it is meant to have
    dec = [s["decisions"] for s in gold["e2e"]["per_sample"].values()]
    assert sum(any(d) for d, _, _, _ in dec) > 10                         # don't-care detections
    assert sum(any(m >= 0 for m in me) for _, _, me, _ in dec) > 100      # matches
    assert sum(any(m >= 0 and m != g for g, m in enumerate(me)) for _, _, me, _ in dec) > 20
