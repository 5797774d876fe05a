from .lexicon import (DeviceLexicon, LexiconMatcher, LexiconTrie, WeightedLexiconMatcher, encode_query, encode_word, lexicon_layout,  # noqa: F401
                      fold_table, load_lexicon, symbol_classes, weighted_cost_tables)
from .pattern import DecodePattern  # noqa: F401
from .weighted_pattern import CharNgramLM, WeightedPattern  # noqa: F401
from .text_evaluator import (TextResultWriter, boxes_to_polygons, find_match_word, find_match_word_weighted,  # noqa: F401
                             instances_to_coco_json, levenshtein, weighted_edit_distance, masks_to_polygons, match_transcript, normalize_detection_line, rotated_boxes_to_polygons)
from .driver import inference_on_dataset  # noqa: F401
from .mask_rings import MaskPolygonizer  # noqa: F401
from .rotated import rotate_ground_truth, rotation_sweep  # noqa: F401
from .ring_check import RingChecker  # noqa: F401
from .ring_simplify import simplify_ring, simplify_rings_host  # noqa: F401
from .rrc_score import (RRCScorer, ThresholdSweep, include_in_dictionary, include_in_dictionary_transcription, load_gt_zip, method_strings,  # noqa: F401
                        parse_detection_line, parse_gt_line, tally_sample, transcription_match)
