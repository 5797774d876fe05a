"""The RRC end-to-end scorer: det.zip + gt.zip -> precision / recall / hmean, end-to-end and detection-only.

A behavioural restatement of the reference's `text_eval_script.evaluate_method` and of the parts of
`rrc_evaluation_funcs` it uses (`load_zip_file` :51-80, `decode_utf8`, the two line parsers :150-302), written from their
behaviour.  The reference scorer itself is never run, here or in the tests: it needs the `Polygon` (GPC) and
`Levenshtein` C packages, which are absent.  Expected values in the tests come from an independent exact checker
(tests/rrc_cases.py: slab decomposition in rational arithmetic).

Split of the work:
  * geometry and decisions on the device (csrc/rrc_score.hip through `ops.native.rrc_pair_areas` / `rrc_match`): the
    area of every polygon, the intersection area of every (ground truth, detection) pair of an image, which detections
    fall on don't-care ground truths, and the greedy IoU matching, for the two care sets;
  * everything that is a string question on the host, in functions that take no tensors: parsing, the don't-care rules
    of word spotting, whether a matched pair's transcriptions agree, and the tallies.

Coordinates.  The writer emits integers and the RRC ground truths are integers, so the scorer takes integral
coordinates only: a token must parse as an integer or as a float with an integral value ("12.0"), with |c| <= 2**20;
anything else raises ValueError.  Rings may have either orientation on the GT side, must be clockwise in image
coordinates on the detection side (what `normalize_detection_line` emits), and are taken to be simple: the reference
does not validate GT rings, and the result for a self-intersecting GT ring is unspecified here.

Two places where the reference's output is an accident are fixed rather than copied: `iouMat` of an image without
ground truths or without detections is `[]` (the reference returns an uninitialised 1x1 array), and exceptions are
ValueError with the reference's wording.
"""
from __future__ import annotations

import io
import re
import zipfile
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from .text_evaluator import normalize_detection_line

MAX_COORD = 1 << 20
WORKSPACE_CAP_BYTES = 256 << 20          # most bytes of `inter` (8 per pair) alive at once; images are chunked to stay under it
MIN_LENGTH_CARE_WORD = 3
IOU_MAT_MAX_DETECTIONS = 100             # per_sample['iouMat'] is [] above this many detections (:447)
SPECIAL_CHARACTERS = "!?.:,*\"()·[]/'"
_DICTIONARY_SEPARATORS = "'!?.:,*\"()·[]/"
_DET_NAME = r"([0-9]+).txt"
_GT_NAME = {"icdar": r"gt_img_([0-9]+).txt", "totaltext": r"([0-9]+).txt"}
_ICDAR_LINE = re.compile(r"^\s*" + r"\s*,\s*".join([r"(-?[0-9]+)"] * 8) + r"\s*,(.*)$")
_QUOTED = re.compile(r'^\s*"(.*)"\s*$')
_LETTER_RANGES = ((ord("a"), ord("z")), (ord("A"), ord("Z")), (ord("À"), ord("ƿ")), (ord("Ǆ"), ord("ɿ")), (ord("Ά"), ord("Ͽ")),
                  (ord("-"), ord("-")))

EVALUATION_PARAMS = {"IOU_CONSTRAINT": 0.5, "AREA_PRECISION_CONSTRAINT": 0.5, "MIN_LENGTH_CARE_WORD": MIN_LENGTH_CARE_WORD,
                     "LTRB": False, "CRLF": False, "CONFIDENCES": False, "SPECIAL_CHARACTERS": SPECIAL_CHARACTERS,
                     "ONLY_REMOVE_FIRST_LAST_CHARACTER": True}


# ----------------------------------------------------------------------------------------------- files and lines (host)

def decode_utf8(raw: bytes) -> str:
    """Bytes of one file -> text: undecodable bytes become U+FFFD, one leading BOM is removed."""
    text = raw.decode("utf-8", "replace")
    return text[1:] if text.startswith("\ufeff") else text


def file_lines(text: str) -> List[str]:
    """The non-empty lines of a file; lines end with LF (CRLF is off in the protocol), stray CR / LF are removed."""
    out = []
    for line in text.split("\n"):
        line = line.replace("\r", "").replace("\n", "")
        if line != "":
            out.append(line)
    return out


def load_zip_entries(file: Union[str, bytes, io.IOBase], name_pattern: str, all_entries: bool = False) -> "OrderedDict[str, bytes]":
    """Entries of a zip whose name matches `name_pattern` (at its start, as `re.match`), keyed by the pattern's first
    group (the digits, as written: '0000012' and '12' are different samples), in archive order.  Other entries are
    skipped, or raise when `all_entries`."""
    if isinstance(file, (bytes, bytearray)):
        file = io.BytesIO(bytes(file))
    try:
        archive = zipfile.ZipFile(file, mode="r", allowZip64=True)
    except Exception as e:
        raise ValueError("Error loading the ZIP archive") from e
    out: "OrderedDict[str, bytes]" = OrderedDict()
    with archive:
        for name in archive.namelist():
            m = re.match(name_pattern, name)
            if m is None:
                if all_entries:
                    raise ValueError("ZIP entry not valid: %s" % name)
                continue
            out[m.group(1) if m.groups() else name] = archive.read(name)
    return out


def parse_coordinate(token: str) -> int:
    """One coordinate: an integer, or a float string with an integral value; |c| <= 2**20."""
    try:
        v = int(token)
    except ValueError:
        f = float(token)                                   # ValueError for anything that is not a number
        if f != f or f in (float("inf"), float("-inf")) or f != int(f):
            raise ValueError(f"coordinate {token!r} is not integral")
        v = int(f)
    if abs(v) > MAX_COORD:
        raise ValueError(f"coordinate {token!r} exceeds 2**20 in magnitude")
    return v


def _unquote(transcription: str) -> str:
    m = _QUOTED.match(transcription)
    if m is not None:
        return m.group(1).replace("\\\\", "\\").replace('\\"', '"')
    return transcription


def _ring(tokens: Sequence[str], line: str) -> List[int]:
    if len(tokens) % 2 != 0:
        raise ValueError(f"num cors should be even: {line!r}")
    return [parse_coordinate(t) for t in tokens]


def parse_gt_line(line: str, line_format: str) -> Tuple[List[int], str]:
    """One ground-truth line -> ([x1, y1, ..., xn, yn], transcription).  'totaltext': `x1,y1,...,xn,yn,####text`;
    'icdar': eight integers, a comma, the transcription (kept as it stands, blanks included).  A transcription in double
    quotes is un-escaped (\\\\ -> \\, \\" -> ")."""
    if line_format == "totaltext":
        parts = line.strip().split(",####")
        if len(parts) < 2:
            raise ValueError(f"no ',####' in line {line!r}")
        points, text = _ring(parts[0].split(","), line), parts[1].strip()
    elif line_format.startswith("icdar"):
        m = _ICDAR_LINE.match(line)
        if m is None:
            raise ValueError("Format incorrect. Should be: x1,y1,x2,y2,x3,y3,x4,y4,transcription")
        points, text = _ring([m.group(i) for i in range(1, 9)], line), m.group(9)
    else:
        raise ValueError(f"unknown line format {line_format!r}")
    return points, _unquote(text)


def parse_detection_line(line: str, validate: bool = True) -> Tuple[List[int], str]:
    """One detection line `x1,y1,...,xn,yn,####text` -> (points, transcription).  The ring must be what
    `normalize_detection_line` emits: at least 3 points, non-zero area, clockwise in image coordinates, and (checked
    when `validate`; quadratic in the number of points) not self-intersecting.  ValueError otherwise."""
    parts = line.strip().split(",####")
    if len(parts) < 2:
        raise ValueError(f"no ',####' in line {line!r}")
    points = _ring(parts[0].split(","), line)
    n = len(points) // 2
    xs, ys = points[0::2], points[1::2]
    area2 = sum(xs[i] * ys[(i + 1) % n] - xs[(i + 1) % n] * ys[i] for i in range(n)) if n >= 3 else 0
    if n < 3 or area2 == 0:
        raise ValueError(f"not a valid polygon: {line!r}")
    if area2 > 0:
        raise ValueError(f"Points are not clockwise: {line!r}")
    if validate:
        cors = ",".join(str(v) for v in points)
        if normalize_detection_line(cors + ",####x") != cors + ",####x":
            raise ValueError(f"polygon has intersecting sides: {line!r}")
    return points, _unquote(parts[1].strip())


# ------------------------------------------------------------------------------------------------ string rules (host)

def _dictionary_form(transcription: str) -> str:
    if transcription[len(transcription) - 2:] in ("'s", "'S"):
        transcription = transcription[:len(transcription) - 2]
    transcription = transcription.strip("-")
    for ch in _DICTIONARY_SEPARATORS:
        transcription = transcription.replace(ch, " ")
    return transcription.strip()


def include_in_dictionary(transcription: str) -> bool:
    """Word spotting: does a ground-truth word count?  After dropping a final 's, outer hyphens and turning the special
    characters into blanks: one word, at least 3 characters, letters of the listed ranges and hyphens only."""
    t = _dictionary_form(transcription)
    if " " in t or len(t) < MIN_LENGTH_CARE_WORD:
        return False
    for ch in t:
        c = ord(ch)
        if ch in "×÷·" or not any(lo <= c <= hi for lo, hi in _LETTER_RANGES):
            return False
    return True


def include_in_dictionary_transcription(transcription: str) -> str:
    """Word spotting: the form in which a kept ground-truth word is compared."""
    return _dictionary_form(transcription)


def transcription_match(gt: str, det: str, special: str = SPECIAL_CHARACTERS) -> bool:
    """End-to-end comparison with ONLY_REMOVE_FIRST_LAST_CHARACTER: equal, or equal after dropping one special character
    from the start and / or the end of the GROUND TRUTH.  An empty ground truth that is not equal to the detection gives
    False (the reference's indexing error, which its caller turns into False)."""
    if gt == det:
        return True
    if gt == "":
        return False
    first, last = gt[0] in special, gt[-1] in special
    return (first and gt[1:] == det) or (last and gt[:-1] == det) or (first and last and gt[1:-1] == det)


def ground_truth_care(transcriptions: Sequence[str], word_spotting: bool) -> Tuple[List[str], List[bool], List[bool]]:
    """(transcriptions as compared, don't-care end-to-end, don't-care detection-only): `###` is don't-care in both sets;
    under word spotting a word that fails `include_in_dictionary` is don't-care end-to-end and a kept word is replaced
    by its dictionary form."""
    out, dc_e2e, dc_det = [], [], []
    for t in transcriptions:
        det_dc = dc = t == "###"
        if word_spotting and not dc:
            if include_in_dictionary(t):
                t = include_in_dictionary_transcription(t)
            else:
                dc = True
        out.append(t)
        dc_e2e.append(dc)
        dc_det.append(det_dc)
    return out, dc_e2e, dc_det


def pair_correct(gt_transcription: str, det_transcription: str, word_spotting: bool) -> bool:
    g = gt_transcription.upper().replace("####", "")
    d = det_transcription.upper()
    return g == d if word_spotting else transcription_match(g, d)


MAX_SWEEP_COMBINATIONS = 1 << 20
ACCEPT_WIDTH = 4                         # a ground truth accepts at most 4 strings: itself, without a first / a last / both special characters
NO_WORD = -2                             # id of a detection string that no ground truth accepts (gt_accept pads with -1)


def accepted_strings(gt_transcription: str, word_spotting: bool) -> List[str]:
    """The detection strings (upper-cased) for which `pair_correct(gt_transcription, det, word_spotting)` holds."""
    g = gt_transcription.upper().replace("####", "")
    out = [g]
    if not word_spotting and g != "":
        first, last = g[0] in SPECIAL_CHARACTERS, g[-1] in SPECIAL_CHARACTERS
        for ok, t in ((first, g[1:]), (last, g[:-1]), (first and last, g[1:-1])):
            if ok and t not in out:
                out.append(t)
    return out


def transcription_ids(samples: Sequence["GroundTruthSample"], det_transcriptions: Sequence[Sequence[str]],
                      word_spotting: bool) -> Tuple[np.ndarray, np.ndarray]:
    """Whether a matched pair is correct, as an integer question: (gt_accept int32 [n_gt, 4] padded with -1, det_word int32
    [n_det]) over the ground truths of `samples` and the detections of `det_transcriptions` (one list per image), both
    flattened in image order, with `det_word[d] in gt_accept[g]` <=> `pair_correct(gt g as compared, detection d,
    word_spotting)` for EVERY pair.  A detection string no ground truth accepts gets NO_WORD.  Takes no tensors."""
    ids: Dict[str, int] = {}
    gts = [t for s in samples for t in s.transcriptions]
    gt_accept = np.full((len(gts), ACCEPT_WIDTH), -1, dtype=np.int32)
    for g, t in enumerate(gts):
        for j, a in enumerate(accepted_strings(t, word_spotting)):
            gt_accept[g, j] = ids.setdefault(a, len(ids))
    det_word = np.fromiter((ids.get(t.upper(), NO_WORD) for image in det_transcriptions for t in image), dtype=np.int32,
                           count=sum(len(image) for image in det_transcriptions))
    return gt_accept, det_word


# ------------------------------------------------------------------------------------------------------- tallies (host)

class GroundTruthSample(NamedTuple):
    points: List[List[int]]
    raw_transcriptions: List[str]
    transcriptions: List[str]          # as compared (word spotting applied)
    dontcare_e2e: List[bool]
    dontcare_det: List[bool]


class SampleCounts(NamedTuple):
    matched: int
    gt_care: int
    det_care: int
    det_only_matched: int
    det_only_gt_care: int
    det_only_det_care: int


def _precision_recall(correct: int, n_gt_care: int, n_det_care: int):
    if n_gt_care == 0:
        recall, precision = float(1), (float(0) if n_det_care > 0 else float(1))
    else:
        recall = float(correct) / n_gt_care
        precision = 0 if n_det_care == 0 else float(correct) / n_det_care
    hmean = 0 if (precision + recall) == 0 else 2.0 * precision * recall / (precision + recall)
    return precision, recall, hmean


def tally_sample(gt: GroundTruthSample, det_points: Sequence[Sequence[int]], det_transcriptions: Sequence[str],
                 match_e2e: Sequence[int], match_det: Sequence[int], det_dontcare_e2e: Sequence[int],
                 det_dontcare_det: Sequence[int], iou_mat, word_spotting: bool) -> Tuple[dict, SampleCounts]:
    """One image's per_sample entry and its contribution to the global sums (:412-455) from the decisions: match_*[g] is
    the detection GT g took (-1: none), det_dontcare_*[d] whether detection d fell on a don't-care GT."""
    n_gt, n_det = len(gt.points), len(det_points)
    correct = sum(1 for g, d in enumerate(match_e2e)
                  if d >= 0 and pair_correct(gt.transcriptions[g], det_transcriptions[d], word_spotting))
    det_only_correct = sum(1 for d in match_det if d >= 0)
    gt_dc = [g for g in range(n_gt) if gt.dontcare_e2e[g]]
    det_dc = [d for d in range(n_det) if det_dontcare_e2e[d]]
    counts = SampleCounts(correct, n_gt - len(gt_dc), n_det - len(det_dc), det_only_correct,
                          n_gt - sum(1 for f in gt.dontcare_det if f), n_det - sum(1 for f in det_dontcare_det if f))
    precision, recall, hmean = _precision_recall(correct, counts.gt_care, counts.det_care)
    sample = {"precision": precision, "recall": recall, "hmean": hmean,
              "iouMat": [] if n_det > IOU_MAT_MAX_DETECTIONS or iou_mat is None else iou_mat,
              "gtPolPoints": [[float(v) for v in p] for p in gt.points],
              "detPolPoints": [[float(v) for v in p] for p in det_points],
              "gtTrans": list(gt.transcriptions), "detTrans": list(det_transcriptions),
              "gtDontCare": gt_dc, "detDontCare": det_dc}
    return sample, counts


def method_strings(counts: Sequence[SampleCounts]) -> Tuple[str, str]:
    """The two method-level lines (:457-465) from the per-image counts."""
    def line(tag, matched, n_gt, n_det):
        recall = 0 if n_gt == 0 else float(matched) / n_gt
        precision = 0 if n_det == 0 else float(matched) / n_det
        hmean = 0 if recall + precision == 0 else 2 * recall * precision / (recall + precision)
        return "{}: precision: {}, recall: {}, hmean: {}".format(tag, precision, recall, hmean)
    tot = [sum(c[k] for c in counts) for k in range(6)]
    return line("E2E_RESULTS", tot[0], tot[1], tot[2]), line("DETECTION_ONLY_RESULTS", tot[3], tot[4], tot[5])


def parse_method_string(line: str) -> Tuple[str, Dict[str, float]]:
    """'E2E_RESULTS: precision: p, recall: r, hmean: h' -> ('E2E_RESULTS', {...}) as `TextEvaluator.evaluate` does."""
    g = re.match(r"(\S+): (\S+): (\S+), (\S+): (\S+), (\S+): (\S+)", line).groups()
    return g[0], {g[i * 2 + 1]: float(g[(i + 1) * 2]) for i in range(3)}


# ----------------------------------------------------------------------------------------------------- ground truth

def gt_line_format(path) -> str:
    return "totaltext" if isinstance(path, str) and ("totaltext" in path or "textocr" in path) else "icdar"


def load_gt_zip(path_or_bytes, line_format: Optional[str] = None) -> "OrderedDict[str, Tuple[List[List[int]], List[str]]]":
    """gt.zip -> {sample key: (rings, transcriptions)} in archive order.  `line_format`: 'icdar' (entries
    gt_img_<n>.txt, eight integers then the transcription) or 'totaltext' (entries <n>.txt, x1,y1,...,xn,yn,####text);
    None: 'totaltext' when the path contains 'totaltext' or 'textocr', else 'icdar', as the reference decides."""
    if line_format is None:
        line_format = gt_line_format(path_or_bytes)
    if line_format not in _GT_NAME:
        raise ValueError(f"unknown line format {line_format!r}")
    out = OrderedDict()
    for key, raw in load_zip_entries(path_or_bytes, _GT_NAME[line_format]).items():
        rings, texts = [], []
        for line in file_lines(decode_utf8(raw)):
            try:
                p, t = parse_gt_line(line, line_format)
            except ValueError as e:
                raise ValueError(f"Line in sample not valid. Sample: {key} Line: {line} Error: {e}") from e
            rings.append(p)
            texts.append(t)
        out[key] = (rings, texts)
    return out


def load_submission(files_or_zip) -> "OrderedDict[str, List[str]]":
    """{file name: [lines]} (TextResultWriter.to_eval_format, normalised) or det.zip (path / bytes) -> {sample key: lines}."""
    out = OrderedDict()
    if isinstance(files_or_zip, dict):
        for name, lines in files_or_zip.items():
            m = re.match(_DET_NAME, name)
            if m is None:
                raise ValueError("ZIP entry not valid: %s" % name)
            out[m.group(1)] = [l for l in (str(x).replace("\r", "").replace("\n", "") for x in lines) if l != ""]
    else:
        for key, raw in load_zip_entries(files_or_zip, _DET_NAME, all_entries=True).items():
            out[key] = file_lines(decode_utf8(raw))
    return out


# ------------------------------------------------------------------------------------------------------------ scorer

class EncodedSubmission(NamedTuple):
    """Device layout of ground truth + one submission (what glass_rrc_pair_areas reads) and the host side of the detections."""
    pts: "object"                       # int32 [P, 2]: GT points, then detection points
    poly_off: "object"                  # int32 [n_gt + n_det + 1]
    gt_off: "object"                    # int32 [I + 1]
    det_off: "object"                   # int32 [I + 1]
    n_gt_per_image: np.ndarray
    n_det_per_image: np.ndarray
    det_points: List[List[List[int]]]   # per image
    det_transcriptions: List[List[str]]


class RRCScorer:
    """Ground truth encoded once and kept on `device`; `score()` evaluates a submission against it.

    gt: what `load_gt_zip` returns, or a gt.zip path / bytes (then `line_format` as in `load_gt_zip`).
    chunk_images: at most this many images per device call (None: as many as fit `workspace_cap_bytes` of `inter`; one
    image larger than the cap is a chunk of its own).  Chunking changes no result.
    ring_checker: a RingChecker (evaluation/ring_check.py); with it the quadratic self-intersection test of `validate=True`
    runs as one batched device check of all lines instead of once per line on the host (same errors for the same lines)."""

    def __init__(self, gt, word_spotting: bool, device, line_format: Optional[str] = None, chunk_images: Optional[int] = None,
                 workspace_cap_bytes: int = WORKSPACE_CAP_BYTES, ring_checker=None):
        import torch
        from ..ops import native as K
        if not isinstance(gt, dict):
            gt = load_gt_zip(gt, line_format)
        self.word_spotting, self.device = bool(word_spotting), torch.device(device)
        self.chunk_images, self.workspace_cap_bytes = chunk_images, int(workspace_cap_bytes)
        self.ring_checker = ring_checker
        if self.device.type != "cuda":
            raise K.GlassLibraryError(f"RRCScorer needs a HIP device (got {self.device}); the geometry has no CPU fallback")
        self.keys: List[str] = list(gt)
        self.samples: List[GroundTruthSample] = []
        for key in self.keys:
            rings, texts = gt[key]
            trans, dc_e2e, dc_det = ground_truth_care(texts, self.word_spotting)
            self.samples.append(GroundTruthSample([list(p) for p in rings], list(texts), trans, dc_e2e, dc_det))
        self._index = {k: i for i, k in enumerate(self.keys)}
        pts, poly_off = _flatten([s.points for s in self.samples])
        self.n_gt_per_image = np.array([len(s.points) for s in self.samples], dtype=np.int64)
        self.n_gt, self.n_gt_points = int(self.n_gt_per_image.sum()), int(pts.shape[0])
        self._gt_pts = K.upload(pts, torch.int32, self.device)
        self._gt_poly_off = poly_off                                                      # host; joined with the detections'
        self._gt_off_host = np.concatenate([[0], np.cumsum(self.n_gt_per_image)]).astype(np.int64)
        self._gt_off = K.upload(self._gt_off_host, torch.int32, self.device)
        flags = lambda k: np.array([f for s in self.samples for f in s[k]], dtype=np.uint8)
        self._gt_dc_e2e = K.upload(flags(3), torch.uint8, self.device)
        self._gt_dc_det = K.upload(flags(4), torch.uint8, self.device)

    def encode_submission(self, files_or_zip, validate: bool = True) -> EncodedSubmission:
        """Parse and check a submission (nothing is launched) and lay it out on the device behind the ground truth."""
        import torch
        from ..ops import native as K
        subm = load_submission(files_or_zip)
        for key in subm:
            if key not in self._index:
                raise ValueError("The sample %s not present in GT" % key)
        det_points: List[List[List[int]]] = [[] for _ in self.keys]
        det_trans: List[List[str]] = [[] for _ in self.keys]
        batched = validate and self.ring_checker is not None
        parsed: List[Tuple[str, str, List[int]]] = []      # (key, line, points) in the order the host path visits them

        def first_crossing() -> None:
            """the error of the first parsed line with crossing sides, as `parse_detection_line(line, True)` words it"""
            verdicts = self.ring_checker.check_flat([p for _, _, p in parsed]) if parsed else []
            for (key, line, _), v in zip(parsed, verdicts):
                if v == 0:                                 # the linear checks passed, so 0 can only be a crossing
                    e = ValueError(f"polygon has intersecting sides: {line!r}")
                    raise ValueError(f"Line in sample not valid. Sample: {key} Line: {line} Error: {e}") from e

        for key, lines in subm.items():
            i = self._index[key]
            for line in lines:
                try:
                    p, t = parse_detection_line(line, validate and not batched)
                except ValueError as e:
                    if batched:
                        first_crossing()                   # a crossing in an earlier line is what the host path stops at
                    raise ValueError(f"Line in sample not valid. Sample: {key} Line: {line} Error: {e}") from e
                if batched:
                    parsed.append((key, line, p))
                det_points[i].append(p)
                det_trans[i].append(t)
        if batched:
            first_crossing()
        pts, poly_off = _flatten(det_points)
        n_det = np.array([len(p) for p in det_points], dtype=np.int64)
        det_off = self.n_gt + np.concatenate([[0], np.cumsum(n_det)])
        all_off = np.concatenate([self._gt_poly_off, self.n_gt_points + poly_off[1:]])
        dev_pts = torch.cat([self._gt_pts, K.upload(pts, torch.int32, self.device)]) if pts.shape[0] else self._gt_pts
        return EncodedSubmission(dev_pts.contiguous(), K.upload(all_off, torch.int32, self.device), self._gt_off,
                                 K.upload(det_off, torch.int32, self.device), self.n_gt_per_image, n_det, det_points, det_trans)

    def chunks(self, n_det_per_image: np.ndarray) -> List[Tuple[int, int]]:
        """[a, b) image ranges with sum G_i * D_i * 8 <= workspace_cap_bytes (and at most chunk_images images) each."""
        pairs = self.n_gt_per_image * n_det_per_image
        cap = max(self.workspace_cap_bytes // 8, 1)
        out, a, acc = [], 0, 0
        for i in range(len(pairs)):
            full = i > a and (acc + int(pairs[i]) > cap or (self.chunk_images is not None and i - a >= self.chunk_images))
            if full:
                out.append((a, i))
                a, acc = i, 0
            acc += int(pairs[i])
        if len(pairs) > a:
            out.append((a, len(pairs)))
        return out

    def score(self, files_or_zip, validate: bool = True) -> dict:
        """Evaluate a submission: the `{name: [lines]}` dict of `TextResultWriter.to_eval_format` after
        `normalize_detection_line`, or det.zip bytes / path.  Returns the reference's result dictionary: 'e2e_method',
        'det_only_method' (the two result lines) and 'per_sample' {key: precision, recall, hmean, iouMat, gtPolPoints,
        detPolPoints, gtTrans, detTrans, gtDontCare, detDontCare, evaluationParams}.  Raises ValueError for a submission
        file that is not in the ground truth and for a line `normalize_detection_line` would drop or reorder
        (`validate=False` skips the quadratic self-intersection test for lines that come straight from it)."""
        import torch
        from ..ops import native as K
        enc = self.encode_submission(files_or_zip, validate)
        G, D = self.n_gt_per_image, enc.n_det_per_image
        g_off, d_off = self._gt_off_host, np.concatenate([[0], np.cumsum(D)])
        params = dict(EVALUATION_PARAMS, WORD_SPOTTING=self.word_spotting)
        per_sample, counts = OrderedDict(), []
        for a, b in self.chunks(D):
            pair_off = np.concatenate([[0], np.cumsum(G[a:b] * D[a:b])]).astype(np.int64)
            n_pairs, n_det = int(pair_off[-1]), int(d_off[b] - d_off[a])
            dev_pair_off = K.upload(pair_off, torch.int64, self.device)
            gt_off, det_off = enc.gt_off[a:b + 1], enc.det_off[a:b + 1]
            area, inter = K.rrc_pair_areas(enc.pts, enc.poly_off, gt_off, det_off, dev_pair_off, n_pairs)
            g0, g1 = int(g_off[a]), int(g_off[b])
            dc_e, dc_d, m_e, m_d = K.rrc_match(area, inter, dev_pair_off, gt_off, det_off, self._gt_dc_e2e[g0:g1],
                                               self._gt_dc_det[g0:g1], n_det)
            dc_e, dc_d, m_e, m_d = (t.cpu().numpy() for t in (dc_e, dc_d, m_e, m_d))
            want_iou = bool(np.any((D[a:b] <= IOU_MAT_MAX_DETECTIONS) & (G[a:b] * D[a:b] > 0)))
            h_area, h_inter = (area.cpu().numpy(), inter.cpu().numpy()) if want_iou else (None, None)
            for i in range(a, b):
                gs, ds = slice(int(g_off[i]) - g0, int(g_off[i + 1]) - g0), slice(int(d_off[i] - d_off[a]), int(d_off[i + 1] - d_off[a]))
                iou = None
                if want_iou and 0 < D[i] <= IOU_MAT_MAX_DETECTIONS and G[i] > 0:
                    p0 = int(pair_off[i - a])
                    iou = iou_matrix(h_inter[p0:p0 + int(G[i] * D[i])].reshape(int(G[i]), int(D[i])),
                                     h_area[int(g_off[i]):int(g_off[i + 1])],
                                     h_area[self.n_gt + int(d_off[i]):self.n_gt + int(d_off[i + 1])]).tolist()
                sample, c = tally_sample(self.samples[i], enc.det_points[i], enc.det_transcriptions[i], m_e[gs].tolist(),
                                         m_d[gs].tolist(), dc_e[ds].tolist(), dc_d[ds].tolist(), iou, self.word_spotting)
                sample["evaluationParams"] = params
                per_sample[self.keys[i]] = sample
                counts.append(c)
        e2e, det_only = method_strings(counts)
        return {"calculated": True, "Message": "", "e2e_method": e2e, "det_only_method": det_only, "per_sample": per_sample}


    def sweep(self, scored_files, text_thresholds, detection_thresholds, validate: bool = True) -> "ThresholdSweep":
        """`score()`'s two result lines for every pair (text_thresholds[i], detection_thresholds[j]) in one pass.
        scored_files: {name: [(line, score_text, score_detection), ...]}, what `TextResultWriter.scored_lines` returns
        after `normalize_detection_line`; in a combination a line is part of the submission iff
        `not (score_text < text_th or score_detection < detection_th)` (fp64, a score equal to the threshold stays), as
        `to_eval_format` decides.  The submission is encoded once and walked in the chunks of `score()`; per chunk the
        pair areas, the don't-care marks and one `rrc_sweep` over all combinations; the counts are read back once.
        `per_sample` is not built.  ValueError as `score()`, and for a bad grid (`threshold_grid`), before any launch."""
        import torch
        from ..ops import native as K
        ts, ds = threshold_grid(text_thresholds, detection_thresholds)
        files, scores = {}, {}
        for name, entries in scored_files.items():
            m = re.match(_DET_NAME, name)
            if m is None:
                raise ValueError("ZIP entry not valid: %s" % name)
            lines = [str(e[0]) for e in entries]
            if any(l.replace("\r", "").replace("\n", "") == "" for l in lines):
                raise ValueError(f"empty line in {name}")
            files[name], scores[m.group(1)] = lines, [(float(e[1]), float(e[2])) for e in entries]
        enc = self.encode_submission(files, validate)
        flat = np.array([p for key in self.keys for p in scores.get(key, [])], dtype=np.float64).reshape(-1, 2)
        if not np.all(np.isfinite(flat)):
            raise ValueError("scores must be finite")
        G, D = self.n_gt_per_image, enc.n_det_per_image
        assert flat.shape[0] == int(D.sum())
        g_off, d_off = self._gt_off_host, np.concatenate([[0], np.cumsum(D)])
        gt_accept, det_word = transcription_ids(self.samples, enc.det_transcriptions, self.word_spotting)
        up = lambda a, t: (K.upload(np.ascontiguousarray(a), t, self.device) if a.size else
                           torch.zeros(a.shape, dtype=t, device=self.device))
        gt_accept, det_word = up(gt_accept, torch.int32).reshape(-1, ACCEPT_WIDTH), up(det_word, torch.int32)
        score_text, score_det = up(flat[:, 0], torch.float64), up(flat[:, 1], torch.float64)
        text_th, det_th = up(np.repeat(ts, ds.size), torch.float64), up(np.tile(ds, ts.size), torch.float64)   # k = i * D + j
        counts = torch.zeros((ts.size * ds.size, 6), dtype=torch.int64, device=self.device)
        for a, b in self.chunks(D):
            pair_off = np.concatenate([[0], np.cumsum(G[a:b] * D[a:b])]).astype(np.int64)
            n_pairs, n_det = int(pair_off[-1]), int(d_off[b] - d_off[a])
            dev_pair_off = K.upload(pair_off, torch.int64, self.device)
            gt_off, det_off = enc.gt_off[a:b + 1], enc.det_off[a:b + 1]
            area, inter = K.rrc_pair_areas(enc.pts, enc.poly_off, gt_off, det_off, dev_pair_off, n_pairs)
            g0, g1, d0, d1 = int(g_off[a]), int(g_off[b]), int(d_off[a]), int(d_off[b])
            dc_e, dc_d, _, _ = K.rrc_match(area, inter, dev_pair_off, gt_off, det_off, self._gt_dc_e2e[g0:g1], self._gt_dc_det[g0:g1], n_det)
            K.rrc_sweep(area, inter, dev_pair_off, gt_off, det_off, self._gt_dc_e2e[g0:g1], self._gt_dc_det[g0:g1], dc_e, dc_d,
                        score_text[d0:d1], score_det[d0:d1], gt_accept[g0:g1], det_word[d0:d1], text_th, det_th, counts,
                        max_dets=int(D[a:b].max()))
        return ThresholdSweep(ts, ds, counts.cpu().numpy().reshape(ts.size, ds.size, 6))


class ThresholdSweep:
    """The protocol's result for every pair of a grid of confidence thresholds (`RRCScorer.sweep`).

    text_thresholds [T], detection_thresholds [D]: the grid as given; counts int64 [T, D, 6]: the global sums in
    `SampleCounts` order; e2e, det_only: {'precision', 'recall', 'hmean'} -> float64 [T, D], from `counts` with the
    operations of `method_strings`, so a cell equals what `parse_method_string` reads from that combination's result line."""

    TASKS = ("E2E_RESULTS", "DETECTION_ONLY_RESULTS")

    def __init__(self, text_thresholds, detection_thresholds, counts: np.ndarray):
        self.text_thresholds = np.asarray(text_thresholds, dtype=np.float64).reshape(-1)
        self.detection_thresholds = np.asarray(detection_thresholds, dtype=np.float64).reshape(-1)
        self.counts = np.asarray(counts, dtype=np.int64).reshape(len(self.text_thresholds), len(self.detection_thresholds), 6)
        self.e2e = self._rates(self.counts[..., 0], self.counts[..., 1], self.counts[..., 2])
        self.det_only = self._rates(self.counts[..., 3], self.counts[..., 4], self.counts[..., 5])

    @classmethod
    def empty(cls) -> "ThresholdSweep":
        return cls(np.zeros(0), np.zeros(0), np.zeros((0, 0, 6), dtype=np.int64))

    @staticmethod
    def _rates(matched: np.ndarray, n_gt: np.ndarray, n_det: np.ndarray) -> Dict[str, np.ndarray]:
        with np.errstate(divide="ignore", invalid="ignore"):
            recall = np.where(n_gt == 0, 0.0, matched / n_gt)
            precision = np.where(n_det == 0, 0.0, matched / n_det)
            hmean = np.where(recall + precision == 0, 0.0, 2 * recall * precision / (recall + precision))
        return {"precision": precision, "recall": recall, "hmean": hmean}

    def results(self, i: int, j: int) -> "OrderedDict[str, Dict[str, float]]":
        """What `TextResultWriter.evaluate(scorer, text_thresholds[i], detection_thresholds[j])` returns."""
        return OrderedDict((task, {k: float(v[i, j]) for k, v in rates.items()})
                           for task, rates in zip(self.TASKS, (self.e2e, self.det_only)))

    def best(self, task: str = "E2E_RESULTS") -> Tuple[float, float, "OrderedDict[str, Dict[str, float]]"]:
        """(text threshold, detection threshold, results) at the first maximum of `task`'s hmean in row-major order."""
        if task not in self.TASKS:
            raise ValueError(f"unknown task {task!r}")
        hmean = (self.e2e if task == self.TASKS[0] else self.det_only)["hmean"]
        if hmean.size == 0:
            raise ValueError("the sweep is empty")
        i, j = np.unravel_index(int(np.argmax(hmean)), hmean.shape)              # argmax: the first maximum
        return float(self.text_thresholds[i]), float(self.detection_thresholds[j]), self.results(int(i), int(j))


def threshold_grid(text_thresholds, detection_thresholds) -> Tuple[np.ndarray, np.ndarray]:
    """The two lists as float64 vectors; ValueError for an empty list, a non-finite value or more than 2^20 combinations."""
    out = []
    for name, values in (("text", text_thresholds), ("detection", detection_thresholds)):
        v = np.asarray(list(values), dtype=np.float64).reshape(-1)
        if v.size == 0:
            raise ValueError(f"no {name} threshold")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"{name} thresholds must be finite: {v.tolist()}")
        out.append(v)
    if out[0].size * out[1].size > MAX_SWEEP_COMBINATIONS:
        raise ValueError(f"{out[0].size} x {out[1].size} combinations, at most 2**20")
    return out[0], out[1]


def iou_matrix(inter: np.ndarray, area_gt: np.ndarray, area_det: np.ndarray) -> np.ndarray:
    """inter / (area_g + area_d - inter), 0 where the union is 0: the same fp64 operations as the device's matching."""
    union = (area_gt[:, None] + area_det[None, :]) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union == 0.0, 0.0, inter / union)


def _flatten(rings_per_image: Sequence[Sequence[Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray]:
    """[[ring, ...] per image] -> (pts int32 [P, 2], poly_off int64 [n_poly + 1]); range-checked."""
    rings = [r for image in rings_per_image for r in image]
    flat = np.fromiter((v for r in rings for v in r), dtype=np.int64, count=sum(len(r) for r in rings))
    if flat.size and int(np.abs(flat).max()) > MAX_COORD:
        raise ValueError("coordinate exceeds 2**20 in magnitude")
    off = np.concatenate([[0], np.cumsum([len(r) // 2 for r in rings], dtype=np.int64)]).astype(np.int64)
    return flat.astype(np.int32).reshape(-1, 2), off
