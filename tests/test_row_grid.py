"""Host: the statement of the rows, cells, tables and columns (glass_amd.postprocess.row_grid.row_grid_host) against the
independent checker of row_grid_cases.py on every case, what the scenes are stated to give, every ValueError, the header, the
config keys, and `rows_of` / `tables_of` / `rows_text` on hand-made Instances."""
import os

import numpy as np
import pytest

import row_grid_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glass_row_grid_workspace_bytes", "glass_row_grid"]
RECEIPT_TEXT = ("ACME STORE\n12 Main Street\nCoffee\t3.50\nSandwich deluxe\t12.00\nwith cheese\nTea\t2.00\nTOTAL\t17.50\nThank you")


def _assert_equal(got, ref, name):
    assert got["row_count"] == ref["row_count"] and got["table_count"] == ref["table_count"], name
    for k in C.INT_FIELDS:
        assert got[k].dtype == np.int32 and got[k].tolist() == ref[k], (name, k)
    for k, n in (("row_boxes", ref["row_count"]), ("table_boxes", ref["table_count"])):
        assert got[k].dtype == np.float32 and got[k].shape == (n, 5), (name, k)
        for b in range(n):
            assert C.box_ulps(got[k][b], ref[k][b]) <= 1, (name, k, b)


def _rows_by_text(name):
    """the rows of a case as lists of cell texts, and its reference"""
    _, boxes, texts, ref = C.case(name)
    rows = [[texts[k] for k in ref["row_order"][a:b]] for a, b in zip(ref["row_start"][:-1], ref["row_start"][1:])]
    return rows, texts, ref


def test_equals_the_checker_on_every_case():
    from glass_amd.postprocess.row_grid import row_grid_host
    tables = multi = 0
    for name, boxes, texts, ref in C.all_cases():
        got = row_grid_host(boxes)
        print(f"[row_grid] {name}: {len(boxes)} lines, {ref['row_count']} rows ({ref['multi_rows']} multi-cell), {ref['table_count']} "
              f"tables, margins {ref['cmp_margin']:.2e} / {ref['key_margin']:.2e}")
        _assert_equal(got, ref, name)
        tables += ref["table_count"] > 1
        multi += 0 < ref["multi_rows"] < ref["row_count"]
    assert tables >= 8 and multi >= 12                                 # the scenes are no trivial ones


def test_the_scenes_come_out_as_stated():
    for name in ("receipt", "receipt at 30 degrees", "receipt at -170 degrees"):
        rows, texts, ref = _rows_by_text(name)
        assert "\n".join("\t".join(r) for r in rows) == RECEIPT_TEXT, name
        by = {t: k for k, t in enumerate(texts)}
        assert [ref["table_id"][by[t]] for t in ("Coffee", "3.50", "Sandwich deluxe", "12.00", "Tea", "2.00")] == [0] * 6, name
        assert [ref["table_id"][by[t]] for t in ("TOTAL", "17.50")] == [1, 1], name
        assert [ref["col_id"][by[t]] for t in ("Coffee", "3.50", "Sandwich deluxe", "12.00", "Tea", "2.00", "TOTAL", "17.50")] == [0, 1] * 4
        assert all(ref["table_id"][by[t]] == -1 and ref["col_id"][by[t]] == -1
                   for t in ("ACME STORE", "12 Main Street", "with cheese", "Thank you")), name
        assert ref["table_rows"] == [3, 1] and ref["table_cols"] == [2, 2], name
    rows, texts, ref = _rows_by_text("4 x 3 table and a 2 x 2 table far below")
    assert rows == [["title"]] + [[f"r{r}c{c}" for c in range(3)] for r in range(4)] + [["footnote"]] + \
        [[f"s{r}c{c}" for c in range(2)] for r in range(2)]
    assert ref["table_rows"] == [4, 2] and ref["table_cols"] == [3, 2]
    assert [ref["table_id"][texts.index(t)] for t in ("title", "footnote", "r0c0", "r3c2", "s0c0", "s1c1")] == [-1, -1, 0, 0, 1, 1]
    assert [ref["col_id"][texts.index(f"r{r}c{c}")] for r in range(4) for c in range(3)] == [0, 1, 2] * 4
    rows, texts, ref = _rows_by_text("7 x 5 table at 30 degrees")
    assert ref["table_rows"] == [7] and ref["table_cols"] == [5] and rows[1] == [f"r0c{c}" for c in range(5)]
    assert _rows_by_text("two tables, close")[2]["table_rows"] == [5]                       # 22 px apart, lines of 20 px: one table
    assert _rows_by_text("two tables, far")[2]["table_rows"] == [3, 2]                      # 47 px apart: beyond 2.0 heights
    rows, texts, ref = _rows_by_text("two prose columns")                                   # the known limit: rows by rule
    assert rows == [[f"c0l{r}", f"c1l{r}"] for r in range(4)] and ref["table_cols"] == [2]
    rows, texts, ref = _rows_by_text("staircase of 1024")                                   # one row of diameter 1023
    assert rows == [[f"s{k}" for k in range(1024)]] and ref["table_cols"] == [1024] and ref["table_rows"] == [1]
    rows, texts, ref = _rows_by_text("diagonal of 1024")                                    # two columns of diameter 511
    assert rows == [[f"r{r}c0", f"r{r}c1"] for r in range(512)] and ref["table_cols"] == [2] and ref["table_rows"] == [512]
    assert [ref["col_id"][texts.index(f"r{r}c1")] for r in (0, 255, 511)] == [1, 1, 1]
    rows, texts, ref = _rows_by_text("diagonal of 129")
    assert rows[0] == ["alone"] and ref["table_rows"] == [64]
    rows, texts, ref = _rows_by_text("singletons, 1023")
    assert rows == [[f"l{k}"] for k in range(1023)] and ref["table_count"] == 0
    rows, texts, ref = _rows_by_text("identical boxes")                                     # not beside each other: no row-mates
    assert ref["row_id"] == list(range(70)) and ref["table_count"] == 0
    rows, texts, ref = _rows_by_text("two lines of one row in one column")
    assert rows == [["A", "B", "D"], ["C", "E"]]
    assert [ref["col_id"][texts.index(t)] for t in "ABCDE"] == [0, 0, 0, 1, 1] and ref["table_cols"] == [2]


def test_known_answers_and_thresholds():
    from glass_amd.postprocess.row_grid import row_grid_host
    empty = row_grid_host(np.zeros((0, 5), dtype=np.float32))
    assert empty["row_count"] == 0 and empty["row_start"].tolist() == [0] and empty["row_boxes"].shape == (0, 5)
    assert empty["table_count"] == 0 and empty["table_boxes"].shape == (0, 5) and empty["table_rows"].shape == (0,)
    one = row_grid_host(np.array([[10, 20, 30, 8, 0]], dtype=np.float32))
    assert one["row_order"].tolist() == [0] and one["row_boxes"].tolist() == [[10.0, 20.0, 30.0, 8.0, 0.0]] and one["table_id"].tolist() == [-1]
    pair = np.array([[300, 100, 80, 20, 0], [100, 104, 120, 20, 0]], dtype=np.float32)      # 16 of 20 px shared: one row
    got = row_grid_host(pair)
    assert got["row_id"].tolist() == [0, 0] and got["row_pos"].tolist() == [1, 0] and got["row_order"].tolist() == [1, 0]
    assert got["row_boxes"].tolist() == [[190.0, 102.0, 300.0, 24.0, 0.0]] and got["table_boxes"].tolist() == got["row_boxes"].tolist()
    assert got["table_id"].tolist() == [0, 0] and got["col_id"].tolist() == [1, 0] and got["table_cols"].tolist() == [2]
    assert row_grid_host(pair, {"row_min_overlap": 0.9})["row_count"] == 2
    pair[1, 3] = 44.0                                                  # 20 / 44 of the taller
    assert row_grid_host(pair)["row_count"] == 2
    assert row_grid_host(pair, {"row_min_height_ratio": 0.4})["row_count"] == 1
    # two rows whose cells share 30 of 100 px along the text and stand 38 px apart
    grid = np.array([[100, 100, 100, 20, 0], [400, 100, 100, 20, 0], [170, 158, 100, 20, 0], [470, 158, 100, 20, 0]], dtype=np.float32)
    assert row_grid_host(grid)["table_rows"].tolist() == [2]
    assert row_grid_host(grid, {"column_min_overlap": 0.4})["table_rows"].tolist() == [1, 1]
    assert row_grid_host(grid, {"table_max_row_gap": 1.5})["table_rows"].tolist() == [1, 1]
    # an invalid line is a row of its own, after the valid ones, its box its own values bit for bit, in no table
    name, boxes, texts, ref = C.case("lines that are no lines")
    got = row_grid_host(boxes)
    bad = [k for k in range(len(boxes)) if not ref["valid"][k]]
    assert len(bad) == 9 and got["row_order"][-9:].tolist() == bad and got["row_pos"][bad].tolist() == [0] * 9
    assert got["table_id"][bad].tolist() == [-1] * 9 and got["col_id"][bad].tolist() == [-1] * 9
    for k in bad:
        assert got["row_boxes"][got["row_id"][k]].view(np.uint32).tolist() == boxes[k].view(np.uint32).tolist()


def test_row_first_counts_the_words_ahead():
    from glass_amd.postprocess.row_grid import row_grid_host
    name, boxes, texts, ref = C.case("page of 129")
    L = len(boxes)
    rng = np.random.RandomState(3)
    start = np.concatenate([[0], np.cumsum(rng.randint(1, 6, size=L))]).astype(np.int32)
    K = int(start[-1])                                                 # K words in L lines: the CSR has K + 1 entries
    start = np.concatenate([start, np.full((K - L,), K, dtype=np.int32)])
    got = row_grid_host(boxes, line_start=start, K=K)
    assert got["row_first"].dtype == np.int32 and got["row_first"].tolist() == C.row_first(ref, start, K)
    sizes = np.diff(start)
    assert got["row_first"][got["row_order"]].tolist() == np.concatenate([[0], np.cumsum(sizes[got["row_order"]])[:-1]]).tolist()
    hostile = start.copy()
    hostile[5], hostile[17], hostile[40] = -4, K + 9, 0
    got = row_grid_host(boxes, line_start=hostile, K=K)
    assert got["row_first"].tolist() == C.row_first(ref, hostile, K)
    assert "row_first" not in row_grid_host(boxes)
    with pytest.raises(ValueError, match="line_start"):
        row_grid_host(boxes, line_start=start[:L])


def test_value_errors():
    from glass_amd.postprocess.row_grid import DEFAULT_PARAMS, check_grid_params, row_grid_host
    boxes = C.shared_column()[0]
    nan, inf = float("nan"), float("inf")
    assert DEFAULT_PARAMS == C.DEFAULTS and check_grid_params() == C.DEFAULTS
    for key in C.DEFAULTS:
        for bad in (nan, inf, -inf, -0.5, "wide", None, True):
            with pytest.raises(ValueError, match=key):
                row_grid_host(boxes, {key: bad})
            with pytest.raises(ValueError, match=key):
                check_grid_params(**{key: bad})
    for key, bad in (("row_min_overlap", 0.0), ("row_min_overlap", 1.0001), ("row_min_height_ratio", 1.0001),
                     ("column_min_overlap", 1.0), ("column_min_overlap", 1.5)):
        with pytest.raises(ValueError, match=key):
            row_grid_host(boxes, {key: bad})
    for good in ({"row_min_overlap": 1.0}, {"row_min_overlap": 1e-6}, {"row_min_height_ratio": 1.0}, {"row_min_height_ratio": 0},
                 {"column_min_overlap": 0}, {"column_min_overlap": 0.999}, {"table_max_row_gap": 0}, {"table_max_row_gap": 1e6}, {}):
        row_grid_host(boxes, good)
    with pytest.raises(ValueError, match="1025 lines"):
        row_grid_host(np.zeros((1025, 5), dtype=np.float32))
    with pytest.raises(TypeError):
        row_grid_host(boxes, {"max_slant": 1.0})
    # the binding refuses before it looks at the device
    from glass_amd.ops import native as K
    import torch
    b, c = torch.zeros((1, 4, 5)), torch.zeros((1,), dtype=torch.int32)
    for key in C.DEFAULTS:
        with pytest.raises(ValueError, match=key):
            K.row_grid(b, c, **{key: nan})
    with pytest.raises(ValueError, match="K <= 1024"):
        K.row_grid(torch.zeros((1, 1025, 5)), c)
    with pytest.raises(ValueError, match="K <= 1024"):
        K.row_grid(torch.zeros((4, 5)), c)
    with pytest.raises(ValueError, match="line_count"):
        K.row_grid(b, torch.zeros((2,), dtype=torch.int32))
    with pytest.raises(ValueError, match="line_start"):
        K.row_grid(b, c, torch.zeros((1, 4), dtype=torch.int32))


def test_feature_header_and_binding():
    import re
    from glass_amd import _lib
    from glass_amd.ops import native as K
    from glass_amd.postprocess import row_grid
    with open(os.path.join(ROOT, "include", "glass_hip_feature_grid.h")) as fh:
        text = fh.read()
    assert '#include "glass_hip.h"' in text
    sigs = _lib.signatures(text)
    assert list(sigs) == NAMES
    assert len(sigs["glass_row_grid"][1]) == 22 and len(sigs["glass_row_grid_workspace_bytes"][1]) == 2
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_grid.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_row_grid" not in fh.read(), other
    assert "glass_hip_feature_grid.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    for word in ("beside(a, b)", "rowmate(a, b)", "colmate(a, b)", "over(a, b)", "all symmetric", "connected components", "multi-cell",
                 "fixed-shape tree sum", "count of smaller keys", "in index order", "a negative gap passes", "rounded to float32 once",
                 "copied bit for bit", "never read", "no float atomics", "without contraction", "bit-identical",
                 "does not depend on its neighbours", "used as an index unchecked", "bounded by K rounds", "diameter K - 1",
                 "Two prose columns", "A cell of several lines is several rows", "A spanning cell", "at angles far from the page's",
                 "row_first[line] + line_pos"):
        assert word in " ".join(text.replace(" *", " ").split()), word   # the contract is stated where the entry points are declared
    assert int(re.search(r"#define GLASS_ROW_GRID_MAX_K (\d+)", text).group(1)) == K.ROW_GRID_MAX_K == row_grid.MAX_LINES
    assert K.ROW_GRID_MAX_K == K.GROUP_LINES_MAX_K == K.ORDER_LINES_MAX_K
    assert _lib.ABI_VERSION == 8
    # the known limits are stated in the module and in README too
    for path in ("glass-text-spotting_amd/glass_amd/postprocess/row_grid.py", "README.md"):
        with open(os.path.join(ROOT, path)) as fh:
            words = " ".join(fh.read().split())
        for word in ("prose columns", "cell of several lines", "spanning cell", "ALIGN_ROWS"):
            assert word in words, (path, word)


def test_config_keys_and_reference_yaml():
    from glass_amd.config import get_glass_cfg
    from glass_amd.postprocess import build_post_processor
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    cfg = get_glass_cfg(path)
    pp = cfg.POST_PROCESSING
    assert pp.ALIGN_ROWS is False
    assert (pp.ROW_MIN_OVERLAP, pp.ROW_MIN_HEIGHT_RATIO, pp.COLUMN_MIN_OVERLAP, pp.TABLE_MAX_ROW_GAP) == (0.5, 0.5, 0.1, 2.0)
    for name in sorted(os.listdir(os.path.join(ROOT, "configs"))):
        with open(os.path.join(ROOT, "configs", name)) as fh:
            assert "ALIGN_ROWS" not in fh.read(), name                 # a file with the reference's keys only still loads
    assert build_post_processor(cfg).grid_params is None
    lines_only = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True])
    assert build_post_processor(lines_only).grid_params is None
    on = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ALIGN_ROWS", True, "POST_PROCESSING.TABLE_MAX_ROW_GAP", 1.5])
    made = build_post_processor(on)
    assert made.grid_params == dict(C.DEFAULTS, table_max_row_gap=1.5) and made.order_params is None   # no need of ORDER_LINES
    with pytest.raises(ValueError, match="GROUP_LINES"):
        build_post_processor(get_glass_cfg(path, ["POST_PROCESSING.ALIGN_ROWS", True]))
    for key, name, bad in (("ROW_MIN_OVERLAP", "row_min_overlap", 0.0), ("ROW_MIN_HEIGHT_RATIO", "row_min_height_ratio", 1.5),
                           ("COLUMN_MIN_OVERLAP", "column_min_overlap", 1.0), ("TABLE_MAX_ROW_GAP", "table_max_row_gap", -1.0)):
        opts = ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ALIGN_ROWS", True, f"POST_PROCESSING.{key}", bad]
        with pytest.raises(ValueError, match=name):
            build_post_processor(get_glass_cfg(path, opts))
        off = get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, f"POST_PROCESSING.{key}", bad])   # unused while the key is off
        assert build_post_processor(off).grid_params is None


def _instances(boxes, texts):
    """hand-made Instances of a case: every blank-separated piece of a line's text is a word (its box the line's), the words
    shuffled; the per-word fields as the post-processor derives them from the host statement"""
    import torch
    from glass_amd.postprocess import row_grid_host
    from glass_amd.structures.core import Instances, RotatedBoxes
    words = [(k, q, w) for k, t in enumerate(texts) for q, w in enumerate(t.split())]
    sizes = [len(t.split()) for t in texts]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    g = row_grid_host(boxes, line_start=start, K=len(words))
    perm = np.random.RandomState(0).permutation(len(words))
    words = [words[p] for p in perm]
    line = np.array([k for k, _, _ in words])
    inst = Instances((1000, 1000))
    inst.pred_boxes = RotatedBoxes(torch.from_numpy(boxes[line]))
    fields = {"pred_row_ids": g["row_id"][line], "pred_row_pos": g["row_pos"][line], "pred_table_ids": g["table_id"][line],
              "pred_col_ids": g["col_id"][line], "pred_row_rank": g["row_first"][line] + np.array([q for _, q, _ in words])}
    tb = np.zeros((len(words), 5), dtype=np.float32)
    has = g["table_id"][line] >= 0
    tb[has] = g["table_boxes"][g["table_id"][line][has]]
    return inst, fields, {"pred_row_boxes": g["row_boxes"][g["row_id"][line]], "pred_table_boxes": tb}, [w for _, _, w in words], g


def test_rows_of_tables_of_and_rows_text_on_hand_made_instances():
    import torch
    from glass_amd.postprocess import rows_of, rows_text, tables_of
    for name in ("receipt", "receipt at 30 degrees", "receipt at -170 degrees"):
        _, boxes, texts, ref = C.case(name)
        inst, ints, floats, words, g = _instances(boxes, texts)
        for k, v in ints.items():
            with pytest.raises(ValueError, match="ALIGN_ROWS"):
                rows_of(inst)
            inst.set(k, torch.from_numpy(np.asarray(v)).long())
        for k, v in floats.items():
            inst.set(k, torch.from_numpy(v))
        assert sorted(inst.pred_row_rank.tolist()) == list(range(len(words)))
        rows = rows_of(inst)
        assert len(rows) == 8 and all("text" not in c for r in rows for c in r["cells"])
        assert [r["table"] for r in rows] == [None, None, 0, 0, None, 0, 1, None]
        assert [[c["col"] for c in r["cells"]] for r in rows] == [[None], [None], [0, 1], [0, 1], [None], [0, 1], [0, 1], [None]]
        assert [[" ".join(words[k] for k in c["words"]) for c in r["cells"]] for r in rows] == \
            [line.split("\t") for line in RECEIPT_TEXT.split("\n")]
        assert rows[3]["box"] == [float(v) for v in g["row_boxes"][3]]
        with pytest.raises(ValueError, match="pred_texts"):
            rows_text(inst)
        with pytest.raises(ValueError, match="pred_texts"):
            tables_of(inst)
        inst.pred_texts = words
        assert rows_text(inst) == RECEIPT_TEXT                          # every item with its amount
        assert rows_text(inst, cell_sep=" | ").split("\n")[3] == "Sandwich deluxe | 12.00"
        tables = tables_of(inst)
        assert [(t["n_rows"], t["n_cols"]) for t in tables] == [(3, 2), (1, 2)]
        assert tables[0]["rows"] == [["Coffee", "3.50"], ["Sandwich deluxe", "12.00"], ["Tea", "2.00"]] and tables[1]["rows"] == [["TOTAL", "17.50"]]
        assert tables[1]["box"] == [float(v) for v in g["table_boxes"][1]]
        keep = torch.tensor([w not in ("12.00", "deluxe", "ACME", "STORE", "TOTAL", "17.50") for w in words])   # filtering keeps the fields in step
        left = inst[keep]
        assert rows_text(left) == "12 Main Street\nCoffee\t3.50\nSandwich\nwith cheese\nTea\t2.00\nThank you"
        assert [t["rows"] for t in tables_of(left)] == [[["Coffee", "3.50"], ["Sandwich", None], ["Tea", "2.00"]]]
    # two lines of one row in one column; a column that lacks a line in a row
    _, boxes, texts, ref = C.case("two lines of one row in one column")
    inst, ints, floats, words, g = _instances(boxes, texts)
    for k, v in ints.items():
        inst.set(k, torch.from_numpy(np.asarray(v)).long())
    for k, v in floats.items():
        inst.set(k, torch.from_numpy(v))
    inst.pred_texts = words
    assert tables_of(inst)[0]["rows"] == [["A B", "D"], ["C", "E"]] and rows_text(inst, " ") == "A B D\nC E"
    assert tables_of(inst[torch.tensor([w != "E" for w in words])])[0]["rows"] == [["A B", "D"], ["C", None]]
    empty = inst[torch.zeros((len(words),), dtype=torch.bool)]
    assert rows_of(empty) == [] and tables_of(empty) == [] and rows_text(empty) == ""
