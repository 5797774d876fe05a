"""Loader / builder of libglass_hip.so (the C-ABI kernel library, include/glass_hip.h).

The product path has NO CPU fallback: `lib()` raises if the shared object is missing or
does not export every declared symbol, and every op wrapper raises if its tensors are not
on a HIP device.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess
from typing import List, Optional

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)                     # glass-text-spotting_amd/
CSRC = os.path.join(_ROOT, "csrc")
INCLUDE = os.path.join(os.path.dirname(_ROOT), "include")
SO_PATH = os.environ.get("GLASS_HIP_LIB") or os.path.join(_ROOT, "libglass_hip.so")   # override: kernel experiments

EXPORTS = [
    "glass_last_error", "glass_abi_version", "glass_device_count", "glass_conv2d_nhwc", "glass_conv2d_nhwc_f16", "glass_conv2d_nhwc_h16", "glass_local_stem_supported", "glass_local_stem_fused", "glass_local_stem_fused_h16", "glass_backbone_stem_supported", "glass_backbone_stem_fused", "glass_conv3x3_winograd43_body_nhwc", "glass_winograd43_splitk_supported", "glass_winograd43_splitk_workspace_bytes", "glass_conv3x3_winograd43_splitk_nhwc", "glass_roi_align_rotated_up2", "glass_conv2d_splitk_supported", "glass_conv2d_splitk_workspace_bytes", "glass_conv2d_nhwc_splitk", "glass_conv3x3_winograd_body_nhwc",
    "glass_pointwise_supported", "glass_pointwise_weight_floats", "glass_pointwise_pack_weights", "glass_conv1x1_pointwise_nhwc",
    "glass_pointwise_split_supported", "glass_pointwise_split_weight_bytes", "glass_pointwise_split_pack_weights", "glass_conv1x1_pointwise_split_nhwc", "glass_pointwise_split_dual_supported", "glass_conv1x1_pointwise_split_dual_nhwc",
    "glass_conv_h16_supported", "glass_conv_h16_weight_halves", "glass_conv_h16_pack_weights", "glass_conv2d_nhwc_h16_packed",
    "glass_winograd_supported", "glass_winograd_block_channels", "glass_winograd_weight_floats", "glass_winograd_pack_weights", "glass_conv3x3_winograd_nhwc",
    "glass_winograd43_supported", "glass_winograd43_weight_floats", "glass_winograd43_pack_weights", "glass_conv3x3_winograd43_nhwc",
    "glass_winograd43_ragged_supported", "glass_conv3x3_winograd43_ragged_nhwc",
    "glass_maxpool2d_nhwc", "glass_maxpool2d_nhwc_h16", "glass_roi_align_rotated_h16", "glass_pixel_shuffle2x_nhwc", "glass_sigmoid_inplace", "glass_paste_rotated_masks", "glass_mul_inplace", "glass_cast_f32_to_f16",
    "glass_preprocess_image", "glass_image_u8hwc_to_chw_resized", "glass_roi_align_rotated",
    "glass_rpn_workspace_bytes", "glass_rpn_topk_decode", "glass_rotated_nms_select", "glass_pairwise_iou_rotated", "glass_detections_finalize", "glass_postprocess_words", "glass_postprocess_words_dense_workspace_bytes", "glass_postprocess_words_dense", "glass_text_argmax", "glass_pack_word_records",
    "glass_box_decode", "glass_gc_attention_inplace", "glass_mean_over_h", "glass_bilstm_workspace_bytes", "glass_bilstm_recurrence",
    "glass_bilstm_persistent_workspace_bytes", "glass_bilstm_recurrence_persistent", "glass_recurrence_status", "glass_recurrence_test_hook",
    "glass_decode_persistent_supported", "glass_decode_persistent_workspace_bytes", "glass_attention_decode_persistent",
    "glass_decode_workspace_bytes", "glass_attention_decode", "glass_decode_step_workspace_bytes", "glass_attention_decode_step",
    "glass_beam_search_workspace_bytes", "glass_beam_search", "glass_forced_decode_workspace_bytes", "glass_forced_decode",
    "glass_lexicon_match_workspace_bytes", "glass_lexicon_match",
    "glass_lexicon_match_weighted_workspace_bytes", "glass_lexicon_match_weighted",
    "glass_rrc_pair_areas_workspace_bytes", "glass_rrc_pair_areas", "glass_rrc_match_workspace_bytes", "glass_rrc_match",
    "glass_rrc_sweep_workspace_bytes", "glass_rrc_sweep",
    "glass_mask_windows", "glass_mask_rings_workspace_bytes", "glass_mask_rings_count", "glass_mask_rings_write",
    "glass_ring_check_tasks", "glass_ring_check",
    "glass_resize_pil_workspace_bytes", "glass_resize_u8_pil", "glass_resize_u8_pil_into_batch",
]


class GlassLibraryError(RuntimeError):
    pass


# Device code is compiled WITHOUT packed-f32 (v_pk_*_f32) and fma_mix instruction selection.  On MI355X / ROCm 7.2 a VOP3P
# instruction whose low-result selector is non-zero (`v_pk_mul_f32 ... op_sel:[0,1]`, hipcc's code for float2 / float4
# arithmetic that crosses halves) returns a wrong low half in lanes 48..63 whenever a wavefront of ANOTHER kernel issues a
# double-rate f16 / bf16 MFMA on the same SIMD - i.e. whenever an fp16-mode step is in flight beside this one (docs/DESIGN_history_r1-r3.md
# "co-resident MFMA erratum"; scripts/micro/pk_vs_convh16.hip reproduces it without any code of this library).  No code
# inside the victim kernel can prevent it, so the instruction class is not generated at all; tests/test_isa_guard.py
# disassembles the built library and fails on any such instruction.  (The host pass prints "'-packed-fp32-ops' is not a
# recognized feature for this target" - harmless: -Xclang reaches both passes.)
DEVICE_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "-Xclang", "-target-feature", "-Xclang", "-fma-mix-insts"]


ABI_VERSION = 8      # what csrc/common.hip glass_abi_version() returns: bumped only on an incompatible change of include/glass_hip.h
                     # (an entry removed or its signature / meaning changed); added entries are found by symbol (lib() checks EXPORTS)


def sources() -> List[str]:
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def source_sha16() -> str:
    """sha256[:16] over the kernel sources (csrc/*.hip, csrc/*.h, include/*.h, in sorted order): identifies the library
    a profile was taken with (profiles/*_pmc_conv_summary.json records it; bench.py refuses stale counters)."""
    import hashlib
    h = hashlib.sha256()
    h.update(" ".join(DEVICE_FLAGS).encode())       # the flags change the code as much as the sources do
    for f in sorted(sources() + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h"))):
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 every csrc/*.hip into libglass_hip.so (in-tree)."""
    srcs = sources()
    deps = srcs + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h")) + [os.path.abspath(__file__)]
    if not force and os.path.exists(SO_PATH) and all(os.path.getmtime(SO_PATH) >= os.path.getmtime(d) for d in deps):
        return SO_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    objdir = os.path.join(_ROOT, "build")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s) + ".o")
        objs.append(o)
        if (not force and os.path.exists(o) and
                all(os.path.getmtime(o) >= os.path.getmtime(d) for d in [s] + deps[len(srcs):])):
            continue
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *DEVICE_FLAGS, "-I", INCLUDE, "-I", CSRC, "-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd))
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise GlassLibraryError(f"hipcc failed on {s}:\n{out.decode(errors='replace')}")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO_PATH] + objs
    subprocess.check_call(cmd)
    return SO_PATH


_LIB: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise GlassLibraryError(
                f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(SO_PATH)
        missing = [s for s in EXPORTS if not hasattr(L, s)]
        if missing:
            raise GlassLibraryError(f"{SO_PATH} lacks symbols {missing}")
        L.glass_last_error.restype = ctypes.c_char_p
        L.glass_rpn_workspace_bytes.restype = ctypes.c_int64
        L.glass_winograd_weight_floats.restype = ctypes.c_size_t
        L.glass_winograd43_weight_floats.restype = ctypes.c_size_t
        L.glass_pointwise_weight_floats.restype = ctypes.c_size_t
        L.glass_pointwise_split_weight_bytes.restype = ctypes.c_size_t
        L.glass_conv_h16_weight_halves.restype = ctypes.c_size_t
        L.glass_bilstm_workspace_bytes.restype = ctypes.c_int64
        L.glass_bilstm_persistent_workspace_bytes.restype = ctypes.c_int64
        L.glass_decode_persistent_workspace_bytes.restype = ctypes.c_int64
        L.glass_decode_workspace_bytes.restype = ctypes.c_int64
        L.glass_decode_step_workspace_bytes.restype = ctypes.c_int64
        L.glass_beam_search_workspace_bytes.restype = ctypes.c_int64
        L.glass_forced_decode_workspace_bytes.restype = ctypes.c_int64
        L.glass_conv2d_splitk_workspace_bytes.restype = ctypes.c_int64
        L.glass_winograd43_splitk_workspace_bytes.restype = ctypes.c_int64
        L.glass_lexicon_match_workspace_bytes.restype = ctypes.c_int64
        L.glass_lexicon_match_weighted_workspace_bytes.restype = ctypes.c_int64
        L.glass_lexicon_match_weighted_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        _p, _i, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        L.glass_lexicon_match_weighted.restype = ctypes.c_int
        L.glass_lexicon_match_weighted.argtypes = [_p, _p, _p, _i, _p, _l, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p, _i, _i,
                                                   _p, _p, _p, _p, _l, _p]
        L.glass_rrc_pair_areas_workspace_bytes.restype = ctypes.c_int64
        L.glass_rrc_match_workspace_bytes.restype = ctypes.c_int64
        L.glass_rrc_sweep_workspace_bytes.restype = ctypes.c_int64
        L.glass_postprocess_words_dense_workspace_bytes.restype = ctypes.c_int64
        L.glass_mask_rings_workspace_bytes.restype = ctypes.c_int64
        L.glass_ring_check_tasks.restype = ctypes.c_int64
        L.glass_resize_pil_workspace_bytes.restype = ctypes.c_int64
        L.glass_resize_u8_pil.restype = ctypes.c_int
        L.glass_resize_u8_pil.argtypes = [_p, _i, _i, _p, _p, _i, _p, _p, _i, _p, _l, _p, _i, _i, _p]
        L.glass_resize_u8_pil_into_batch.restype = ctypes.c_int
        L.glass_resize_u8_pil_into_batch.argtypes = [_p, _i, _i, _p, _p, _i, _p, _p, _i, _p, _l, _i, _i, _p, _p, _i, _p, _i, _i, _i, _p]
        _LIB = L
    return _LIB


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().glass_last_error().decode(errors="replace")
        raise GlassLibraryError(f"{what or 'glass call'} failed ({rc}): {msg}")
