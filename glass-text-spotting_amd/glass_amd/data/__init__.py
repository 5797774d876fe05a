"""Test-time data path of the evaluation protocol (reference glass/data/): the size rule and PIL-bilinear arithmetic of
detectron2's ResizeShortestEdge, and the inference half of `DatasetMapper`."""
from .dataset_mapper import DatasetMapper  # noqa: F401
from .transforms import (ResizeShortestEdge, RotationTransform, pil_bilinear_coeffs, pil_resize_u8_host,  # noqa: F401
                         rotate_u8_host)
