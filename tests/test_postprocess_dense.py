"""CPU: the float64 reference of the word post-processor and its case builders (tests/postprocess_dense_cases.py), and the
interface of the dense kernel (glass_postprocess_words_dense) as far as it can be checked without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import postprocess_dense_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_reference_reproduces_the_reference_post_processors_golden(case, golden_dir):
    """tests/golden/postprocess.npz is the output of the reference's own PostProcessorRotatedBoxes; same tolerances as
    test_gpu_e_host_tail.py::test_rotated_box_postprocessor_matches_reference_golden holds the kernel to"""
    g = np.load(os.path.join(golden_dir, "postprocess.npz"))
    out = C.reference_image(g[f"{case}_in_boxes"], g[f"{case}_in_scores"], check=False)
    assert len(out["scores"]) == len(g[f"{case}_out_scores"])
    np.testing.assert_allclose(out["scores"], g[f"{case}_out_scores"], atol=1e-6)
    np.testing.assert_allclose(out["boxes"], g[f"{case}_out_boxes"], rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(out["polygons"], g[f"{case}_out_polygons"], rtol=1e-4, atol=5e-3)


@pytest.mark.parametrize("name", list(C.CASE_SPECS))
def test_case_builder_meets_its_margins(name):
    """build_case raises when an image cannot be drawn inside the margins or lacks the structure its kind promises; the
    returned reference was computed with every margin check on"""
    case = C.build_case(name)
    seed, K, counts, kind, scale, T = C.CASE_SPECS[name]
    assert case["boxes"].shape == (len(counts), K, 5) and case["text"].shape == (len(counts), K, T, C.CLASSES)
    for n, (count, ref) in enumerate(zip(counts, case["ref"])):
        again = C.reference_image(case["boxes"][n, :count], case["scores"][n, :count], case["text"][n, :count], scale, check=True)
        assert np.array_equal(again["src"], ref["src"]) and np.array_equal(again["boxes"], ref["boxes"])
        assert not case["boxes"][n, count:].any() and not case["scores"][n, count:].any()
        assert len(ref["scores"]) <= count
        if count >= 64:
            assert 0 < len(ref["scores"]) < count                      # the filters and thresholds all remove something
            assert (ref["text_len"] == T).any() and (ref["text_len"] < T).any()      # words without and with a stop symbol


def test_cases_cover_every_boundary_of_the_dense_kernel():
    counts = {c for name in C.DENSE_CASES for c in C.CASE_SPECS[name][2]}
    assert {0, 1, 128, 129, 192, 193, 256, 257, 512, 513, 1023, 1024} <= counts
    assert {C.CASE_SPECS[name][1] for name in C.DENSE_CASES} == {129, 300, 1024}
    for kind in ("mixed", "sparse"):
        sub = [C.CASE_SPECS[n] for n in C.DENSE_CASES if C.CASE_SPECS[n][3] == kind]
        assert {c for s in sub for c in s[2]} >= {128, 129, 192, 193, 256, 257, 512, 513, 1023, 1024}
    for c in (128, 129, 192, 193, 256, 257, 512, 513, 1023, 1024):
        specs = [s for n, s in C.CASE_SPECS.items() if n in C.DENSE_CASES and c in s[2]]
        assert {s[5] for s in specs} == {26, 51}                         # T
        assert {s[4] is None for s in specs} == {True, False}            # un-scaling off and on
    assert all(C.CASE_SPECS[n][1] <= 128 for n in C.SMALL_CASES)


def test_dense_entry_points_are_declared_and_exported():
    from glass_amd import _lib
    header = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("glass_postprocess_words_dense", "glass_postprocess_words_dense_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8                                          # additive change
    src = open(os.path.join(ROOT, "glass-text-spotting_amd", "csrc", "postprocess_dense.hip")).read()
    assert 'extern "C" int glass_postprocess_words_dense(' in src and "fp contract(off)" in src


def test_python_refuses_more_than_1024_detections_before_any_launch():
    """CPU tensors: a launch (or any device check) would raise GlassLibraryError, the width check comes first"""
    from glass_amd.ops import native as K
    assert K.POSTPROCESS_LDS_MAX_K == 128 and K.POSTPROCESS_MAX_K == 1024
    with pytest.raises(ValueError, match="1024"):
        K.postprocess_words(torch.zeros((1, 1025, 5)), torch.zeros((1, 1025)), torch.zeros((1,), dtype=torch.int32), None, None,
                            list(C.THRESHOLDS), C.STOP)
