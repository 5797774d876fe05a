"""Loader / builder of libglass_hip.so (the C-ABI kernel library, include/glass_hip.h).

The header is the one description of the ABI: `signatures()` parses its prototypes, `EXPORTS` is their names, and `lib()`
gives every entry its `restype` / `argtypes` from them - ctypes then converts plain ints, floats and `None`, passes 64-bit
sizes and device addresses whole, and refuses a wrongly typed argument on the host (`ctypes.ArgumentError`).

One header per feature: include/glass_hip.h is closed (its set of prototypes, `EXPORTS`, is pinned by the host tests), and
so is include/glass_hip_ext.h (`EXT_EXPORTS`, the lexicon beam search).  Every later feature declares its entry points in a
header of its own, include/glass_hip_ext_<feature>.h, which includes the first; `addon_signatures()` parses all of them in
sorted order and `ADDON_EXPORTS` lists their names (a name declared twice is an error).  That set is pinned by the host tests
too (the views header alone), so it is closed as well: a feature after it declares its entry points in
include/glass_hip_feature_<feature>.h (`feature_signatures()`, `FEATURE_EXPORTS`, same rules), and a test pins only the names
of its own header.  `lib()` requires and binds the four sets the same way; additions leave `ABI_VERSION` alone.

The product path has NO CPU fallback: `lib()` raises if the shared object is missing or
does not export every declared symbol, and every op wrapper raises if its tensors are not
on a HIP device.
"""
from __future__ import annotations

import ctypes
import glob
import os
import re
import subprocess
from typing import Dict, List, Optional, Tuple

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)                     # glass-text-spotting_amd/
CSRC = os.path.join(_ROOT, "csrc")
INCLUDE = os.path.join(os.path.dirname(_ROOT), "include")
SO_PATH = os.environ.get("GLASS_HIP_LIB") or os.path.join(_ROOT, "libglass_hip.so")   # override: kernel experiments


class GlassLibraryError(RuntimeError):
    pass


_RESTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_ARGTYPES = {"glass_stream_t": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
             "float": ctypes.c_float, "double": ctypes.c_double}
_SIGNATURES: Optional[Dict[str, Tuple[object, list]]] = None


def signatures(header: Optional[str] = None) -> Dict[str, Tuple[object, list]]:
    """{name: (restype, [argtypes])} of every glass_* prototype of include/glass_hip.h (parsed once), or of the header text
    given.  A prototype starts in column 0 with its return type and may span lines; any parameter with a `*` and
    glass_stream_t are c_void_p (which also takes `ctypes.byref(desc)` and ctypes arrays).  Nothing has a default: a return
    or parameter type not listed above (a struct by value, a new typedef) raises, and so does a `glass_*(` name for which
    no prototype was parsed."""
    global _SIGNATURES
    if header is None:
        if _SIGNATURES is None:
            with open(os.path.join(INCLUDE, "glass_hip.h")) as fh:
                _SIGNATURES = signatures(fh.read())
        return _SIGNATURES
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sigs = {}
    for ret, name, params in re.findall(r"^(\w[\w \t*]*?)\s*\b(glass_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RESTYPES:
            raise GlassLibraryError(f"include/glass_hip.h: {name} returns {ret!r}, which the binding does not know")
        argtypes = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            words = [t for t in prm.split() if t != "const"]
            if "*" in prm:
                argtypes.append(ctypes.c_void_p)
            elif len(words) == 2 and words[0] in _ARGTYPES and "[" not in prm:
                argtypes.append(_ARGTYPES[words[0]])
            else:
                raise GlassLibraryError(f"include/glass_hip.h: {name} has parameter {' '.join(prm.split())!r}, "
                                        "which the binding does not know")
        sigs[name] = (_RESTYPES[ret], argtypes)
    unparsed = sorted(set(re.findall(r"\b(glass_\w+)\s*\(", text)) - set(sigs))
    if unparsed:
        raise GlassLibraryError(f"include/glass_hip.h: no prototype parsed for {unparsed}")
    return sigs


EXPORTS = list(signatures())        # every entry point the header declares, in its order

_EXT_SIGNATURES: Optional[Dict[str, Tuple[object, list]]] = None


def ext_signatures() -> Dict[str, Tuple[object, list]]:
    """`signatures()` of include/glass_hip_ext.h, the header of the entry points added after glass_hip.h was closed"""
    global _EXT_SIGNATURES
    if _EXT_SIGNATURES is None:
        with open(os.path.join(INCLUDE, "glass_hip_ext.h")) as fh:
            _EXT_SIGNATURES = signatures(fh.read())
        both = sorted(set(_EXT_SIGNATURES) & set(signatures()))
        if both:
            raise GlassLibraryError(f"include/glass_hip_ext.h declares {both} again")
    return _EXT_SIGNATURES


EXT_EXPORTS = list(ext_signatures())        # every entry point include/glass_hip_ext.h declares, in its order

_ADDON_SIGNATURES: Optional[Dict[str, Tuple[object, list]]] = None


def addon_headers() -> List[str]:
    """the per-feature headers include/glass_hip_ext_<feature>.h, in sorted order"""
    return sorted(glob.glob(os.path.join(INCLUDE, "glass_hip_ext_*.h")))


def _declared_once(paths: List[str], taken: Dict[str, str]) -> Dict[str, Tuple[object, list]]:
    """`signatures()` of the headers `paths` together; raises for a name in `taken` ({name: header}) or declared by two of them"""
    sigs: Dict[str, Tuple[object, list]] = {}
    for path in paths:
        with open(path) as fh:
            here = signatures(fh.read())
        both = sorted(set(here) & set(taken))
        if both:
            raise GlassLibraryError(f"include/{os.path.basename(path)} declares {both} again (first in "
                                    f"include/{taken[both[0]]})")
        taken.update({n: os.path.basename(path) for n in here})
        sigs.update(here)
    return sigs


def addon_signatures() -> Dict[str, Tuple[object, list]]:
    """`signatures()` of every include/glass_hip_ext_<feature>.h together; a name that two headers declare (one of them may be
    glass_hip.h or glass_hip_ext.h) raises"""
    global _ADDON_SIGNATURES
    if _ADDON_SIGNATURES is None:
        taken = {**{n: "glass_hip.h" for n in signatures()}, **{n: "glass_hip_ext.h" for n in ext_signatures()}}
        _ADDON_SIGNATURES = _declared_once(addon_headers(), taken)
    return _ADDON_SIGNATURES


ADDON_EXPORTS = list(addon_signatures())    # every entry point the per-feature headers declare, header by header

_FEATURE_SIGNATURES: Optional[Dict[str, Tuple[object, list]]] = None


def feature_headers() -> List[str]:
    """the headers include/glass_hip_feature_<feature>.h, in sorted order"""
    return sorted(glob.glob(os.path.join(INCLUDE, "glass_hip_feature_*.h")))


def feature_signatures() -> Dict[str, Tuple[object, list]]:
    """`signatures()` of every include/glass_hip_feature_<feature>.h together; a name that any other header declares raises"""
    global _FEATURE_SIGNATURES
    if _FEATURE_SIGNATURES is None:
        taken = {**{n: "glass_hip.h" for n in signatures()}, **{n: "glass_hip_ext.h" for n in ext_signatures()},
                 **{n: "a glass_hip_ext_*.h" for n in addon_signatures()}}
        _FEATURE_SIGNATURES = _declared_once(feature_headers(), taken)
    return _FEATURE_SIGNATURES


FEATURE_EXPORTS = list(feature_signatures())    # every entry point the glass_hip_feature_*.h headers declare, header by header


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
        missing = [s for s in EXPORTS + EXT_EXPORTS + ADDON_EXPORTS + FEATURE_EXPORTS if not hasattr(L, s)]
        if missing:
            raise GlassLibraryError(f"{SO_PATH} lacks symbols {missing}")
        for name, (restype, argtypes) in {**signatures(), **ext_signatures(), **addon_signatures(), **feature_signatures()}.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().glass_last_error().decode(errors="replace")
        raise GlassLibraryError(f"{what or 'glass call'} failed ({rc}): {msg}")
