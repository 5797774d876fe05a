from .post_processor_rotated_boxes import POST_PROCESSOR_REGISTRY, build_post_processor  # noqa: F401
from . import post_processor_academic  # noqa: F401  (registers PostProcessorAcademic)
from .line_grouping import group_lines_host, lines_of  # noqa: F401
from .line_order import blocks_of, check_order_params, order_lines_host, page_text  # noqa: F401
from .row_grid import check_grid_params, row_grid_host, rows_of, rows_text, tables_of  # noqa: F401
from .char_boxes import char_quads, char_spans_host, chars_of  # noqa: F401
