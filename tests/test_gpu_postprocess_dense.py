"""GPU: the dense word post-processor (glass_postprocess_words_dense, 128 < K <= 1024 padded detections per image) against
the all-in-LDS kernel where both apply, against the float64 reference of tests/postprocess_dense_cases.py above 128, against
the pinned host path, and through the model, the runner and the word records."""
import os

import numpy as np
import pytest
import torch

import postprocess_dense_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("boxes", "scores", "polygons", "src", "char", "text_score", "text_len", "count")


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), list(opts))


def _run(case, thresholds=C.THRESHOLDS, stop=C.STOP):
    from glass_amd.ops import native as K
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = K.postprocess_words(t(case["boxes"]), t(case["scores"]), t(case["counts"]), t(case["text"]), t(case.get("scale_xy")),
                              [float(v) for v in thresholds], stop)
    assert tuple(out) == FIELDS
    return {k: v.cpu() for k, v in out.items()}


def _assert_same_bits(lds, dense, K0, what):
    """the eight outputs identical on the first K0 slots, zero beyond K0 and beyond the counts"""
    assert torch.equal(lds["count"], dense["count"]), what
    for k in FIELDS[:-1]:
        a, d = lds[k], dense[k]
        assert a.dtype == d.dtype
        assert torch.equal(a, d[:, :K0]), (what, k)                       # floats included: same arithmetic, same order
        assert np.array_equal(a.numpy().view(np.uint8), d[:, :K0].contiguous().numpy().view(np.uint8)), (what, k)
        assert not d[:, K0:].any(), (what, k)
        for n, c in enumerate(lds["count"].tolist()):
            assert not d[n, c:].any() and not a[n, c:].any(), (what, k, n)


def test_same_bits_as_the_lds_kernel_where_both_apply(golden_dir):
    """every scene of the regression fixture and the <= 128-box cases: as they are through glass_postprocess_words, zero-padded
    to K = 129 and K = 300 through glass_postprocess_words_dense"""
    from glass_amd.utils.synth import pattern_text
    g = np.load(os.path.join(golden_dir, "postprocess_words_regression.npz"))
    scenes = []
    for name in sorted({k.split("/")[0] for k in g.files}):
        sc = g[f"{name}/in_scores"]
        scenes.append((name, {"boxes": g[f"{name}/in_boxes"], "scores": sc, "counts": g[f"{name}/in_counts"].astype(np.int32),
                              "text": pattern_text(*sc.shape).numpy(), "K": sc.shape[1],
                              "scale_xy": g[f"{name}/in_scale_xy"] if f"{name}/in_scale_xy" in g.files else None},
                       [float(v) for v in g[f"{name}/thresholds"]]))
    assert len(scenes) == 5
    scenes += [(name, C.build_case(name), C.THRESHOLDS) for name in C.SMALL_CASES]
    for name, case, thr in scenes:
        K0 = case["K"]
        assert K0 <= 128
        lds = _run(case, thr)
        assert int(lds["count"].sum()) > 0
        for K in (129, 300):
            _assert_same_bits(lds, _run(C.pad_case(case, K), thr), K0, f"{name} padded to {K}")
        print(f"[dense = LDS bits] {name}: K {K0} -> 129, 300; kept {lds['count'].tolist()}")


def _assert_matches_reference(out, case, what):
    worst = {"boxes": 0.0, "polygons": 0.0, "text_score": 0.0}
    T = case["T"]
    assert out["count"].tolist() == [len(r["scores"]) for r in case["ref"]], what
    for n, ref in enumerate(case["ref"]):
        c = len(ref["scores"])
        assert np.array_equal(out["src"][n, :c].numpy(), ref["src"]), (what, n)
        assert np.array_equal(out["char"][n, :c, :T].numpy(), ref["char"]), (what, n)
        assert np.array_equal(out["text_len"][n, :c].numpy(), ref["text_len"]), (what, n)
        assert np.array_equal(out["scores"][n, :c].numpy().astype(np.float64), ref["scores"]), (what, n)     # copies: exact
        for k in FIELDS[:-1]:
            assert not out[k][n, c:].any(), (what, n, k)
        if c == 0:
            continue
        db = float(np.abs(out["boxes"][n, :c].numpy().astype(np.float64) - ref["boxes"]).max())
        dp = float(np.abs(out["polygons"][n, :c].numpy().astype(np.float64) - ref["polygons"]).max())
        dt = float((np.abs(out["text_score"][n, :c].numpy().astype(np.float64) - ref["text_score"]) / ref["text_score"]).max())
        worst = {"boxes": max(worst["boxes"], db), "polygons": max(worst["polygons"], dp), "text_score": max(worst["text_score"], dt)}
    print(f"[dense vs float64 reference] {what}: kept {out['count'].tolist()} of {case['counts'].tolist()}, max |dbox| = "
          f"{worst['boxes']:.3e}, max |dpolygon| = {worst['polygons']:.3e} px, max rel dtext_score = {worst['text_score']:.3e}")
    # 5e-4 px: the bar test_gpu_e_host_tail.py holds the LDS kernel to against host_call; rtol 1e-5 on the word score, as there
    assert worst["boxes"] <= 5e-4 and worst["polygons"] <= 5e-4 and worst["text_score"] <= 1e-5, (what, worst)


@pytest.mark.parametrize("name", C.DENSE_CASES)
def test_dense_kernel_matches_the_float64_reference(name):
    case = C.build_case(name)
    assert case["K"] > 128
    _assert_matches_reference(_run(case), case, name)


def test_small_cases_match_the_float64_reference_through_both_kernels():
    for name in C.SMALL_CASES:
        case = C.build_case(name)
        _assert_matches_reference(_run(case), case, f"{name} (LDS kernel)")
        _assert_matches_reference(_run(C.pad_case(case, 129)), dict(case, K=129), f"{name} (dense kernel)")


@pytest.mark.parametrize("count", [300, 600])
def test_academic_postprocessor_equals_host_restatement_above_128_boxes(count):
    """PostProcessorAcademic.__call__ (K = n > 128: the dense kernel) vs host_call, with the assertions of
    test_gpu_e_host_tail.py::test_device_postprocessor_equals_host_restatement_with_text"""
    from glass_amd.postprocess import build_post_processor
    from glass_amd.postprocess.post_processor_academic import get_instances_text
    from glass_amd.structures.core import Instances, RotatedBoxes
    dev = torch.device("cuda:0")
    pp = build_post_processor(_cfg(["POST_PROCESSING.TEXT_THRESHOLD", 0.01]))
    b, s, _, ref, _ = C.draw_image((51, count), count, "mixed", None, count, 26)
    b, s = torch.from_numpy(b), torch.from_numpy(s)
    n = len(b)
    g = torch.Generator().manual_seed(count)
    logits = torch.randn((n, 26, 97), generator=g) * 6
    logits[:, 3 + count % 5, 1] += 30.0              # a stop symbol somewhere
    tp = torch.softmax(logits, -1)

    def mk():
        inst = Instances((3000, 3000))
        inst.pred_boxes = RotatedBoxes(b.clone().to(dev))
        inst.scores = s.clone().to(dev)
        inst.pred_classes = torch.zeros(n, dtype=torch.int64, device=dev)
        inst.orientations = torch.stack([torch.arange(n).float(), s], 1).to(dev)
        inst.pred_text_prob = tp.clone().to(dev)
        return inst
    host = pp.host_call(mk())
    devr = pp(mk())
    assert len(host) == len(devr) and ref["stats"]["n0"] > len(host) > 128
    db = np.abs(devr.pred_boxes.tensor.cpu().numpy() - host.pred_boxes.tensor.cpu().numpy())
    dp = np.abs(devr.pred_polygons.cpu().numpy() - host.pred_polygons.cpu().numpy())
    print(f"[post-processor device vs host] {count} boxes: n = {len(host)}, max |dbox| = {db.max():.3e}, max |dpolygon| = {dp.max():.3e} px")
    np.testing.assert_allclose(devr.pred_boxes.tensor.cpu().numpy(), host.pred_boxes.tensor.cpu().numpy(), rtol=0, atol=5e-4)
    np.testing.assert_allclose(devr.scores.cpu().numpy(), host.scores.cpu().numpy(), atol=1e-6)
    np.testing.assert_allclose(devr.pred_polygons.cpu().numpy(), host.pred_polygons.cpu().numpy(), rtol=0, atol=5e-4)
    assert torch.equal(devr.orientations.cpu(), host.orientations.cpu())
    assert torch.equal(devr.pred_text_prob.cpu(), host.pred_text_prob.cpu())
    texts, tscores, _ = get_instances_text(host.pred_text_prob, pp.text_encoder)
    assert devr.pred_texts == texts
    np.testing.assert_allclose(devr.pred_text_scores.cpu().numpy(), np.array(tscores, dtype=np.float32), rtol=1e-5, atol=1e-7)


def test_dense_kernel_is_deterministic():
    case = C.build_case("k1024_cascade")
    assert case["ref"][0]["stats"]["iters"] >= 3
    a, b = _run(case), _run(case)
    for k in FIELDS:
        assert np.array_equal(a[k].numpy().view(np.uint8), b[k].numpy().view(np.uint8)), k
    assert int(a["count"][0]) == len(case["ref"][0]["scores"])


def test_model_results_do_not_depend_on_detections_per_image():
    """the same model and images with TEST.DETECTIONS_PER_IMAGE 128 (LDS kernel) and 300 (dense kernel): no image has more than
    128 raw detections, so the padded width is the only difference and the instances must be the same bit for bit"""
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_image, make_state_dict
    sd = make_state_dict(1234)
    imgs = [make_image(5, 100, 80).numpy(), make_image(9, 100, 80).numpy()]
    runs = []
    for dpi in (128, 300):
        cfg = _cfg(["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "MODEL.DEVICE", "cuda:0", "TEST.DETECTIONS_PER_IMAGE", dpi,
                    "MODEL.RPN.POST_NMS_TOPK_TEST", 300, "POST_PROCESSING.TEXT_THRESHOLD", 0.0])
        runner = GlassRunner(None, None, cfg=cfg, state_dict=sd, post_process=True)
        out = runner.run_batch(imgs)
        det = runner.model.last_batch
        assert det.scores.shape[1] == dpi and max(det.counts_host) <= 128 and sum(det.counts_host) > 0
        runs.append((out, list(det.counts_host)))
    (a, ca), (b, cb) = runs
    assert ca == cb
    assert sum(len(x) for x in a) > 0
    for x, y in zip(a, b):
        assert len(x) == len(y)
        assert torch.equal(x.pred_boxes.tensor, y.pred_boxes.tensor) and torch.equal(x.scores, y.scores)
        assert torch.equal(x.pred_polygons, y.pred_polygons) and torch.equal(x.pred_text_prob, y.pred_text_prob)
        assert x.pred_texts == y.pred_texts


def test_word_records_round_trip_300_boxes():
    from glass_amd.distributed import pack_words, unpack_words
    case = C.build_case("k300_mixed")
    from glass_amd.ops import native as K
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)
    words = K.postprocess_words(t(case["boxes"]), t(case["scores"]), t(case["counts"]), t(case["text"]), None, list(C.THRESHOLDS), C.STOP)
    T = case["T"]
    chars = [chr(33 + i) for i in range(C.CLASSES)]
    got = unpack_words(pack_words(words, 300, T).cpu(), 300, T, chars)
    assert max(len(r["scores"]) for r in case["ref"]) > 128
    for n, (w, ref) in enumerate(zip(got, case["ref"])):
        c = int(words["count"][n])
        assert c == len(ref["scores"]) == len(w["scores"])
        assert torch.equal(w["boxes"], words["boxes"][n, :c].cpu()) and torch.equal(w["scores"], words["scores"][n, :c].cpu())
        assert torch.equal(w["text_scores"], words["text_score"][n, :c].cpu())
        assert torch.equal(w["polygons"], words["polygons"][n, :c].cpu())
        assert w["texts"] == ["".join(chars[i] for i in ref["char"][j][:ref["text_len"][j]]) for j in range(c)]
