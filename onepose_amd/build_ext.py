"""Build libgatsspg_hip.so (matcher), libspp_hip.so (SuperPoint extractor), libpnp_hip.so (RANSAC-EPnP), libsuperglue_hip.so
(SuperGlue 2D-2D matcher), libdet_hip.so (2D object detector tail) and libmap_hip.so (object database builder) in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m onepose_amd.build_ext [--force] [--remarks] [--profiling] [--tuning]

The product libraries never read the environment.  ``--tuning`` builds SEPARATE libraries (``lib*_tuning.so``, never
loaded by the package) with -DGATSSPG_TUNING / -DSPP_TUNING, which read GATSSPG_<KNOB> / SPP_<KNOB> environment variables
(tools/ab_tuning.py; the matcher's knobs are the shape thresholds between two product kernels); ``--profiling`` adds the
mlp0 / split-loop timeline hooks (tools/trace_mlp0.py, tools/trace_sp.py) to such a separate library as well.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")


def _include(*parts):
    return os.path.join("..", "..", "include", *parts)


class Library:
    """One shared library: its sources and headers (relative to csrc/) and whether it has a -DGATSSPG_TUNING / -DSPP_TUNING
    variant (the others have no tuning knobs)."""

    def __init__(self, name, sources, headers, tuning=False):
        self.path = os.path.join(LIB_DIR, f"lib{name}_hip.so")
        self.sources, self.headers, self.tuning = sources, headers, tuning


# The SuperGlue, detector and mapping sources live in csrc/superglue/, csrc/detector/, csrc/mapping/ and their include/ twins: source_hash() (top-level
# files only) does not see them.
LIBRARIES = (
    Library("gatsspg", ["gatsspg_gemm_kernels.hip", "gatsspg_split_kernels.hip", "gatsspg_stream_kernels.hip", "gatsspg_capi.hip",
                        "gatsspg_train_kernels.hip",        # the training head (gtr_*, include/gatsspg_train.h) lives in the matcher's library
                        "gatsspg_trainset_kernels.hip"],    # and the training-set builder (gts_*, include/gatsspg_trainset.h) next to it
            ["gatsspg_common.h", "gatsspg_launch.h", "gatsspg_epilogue.h", "gemm_f32_mfma.h", "gemm_split_glds.h", "capi_common.h",
             "wg_primitives.h", "ransac_sample.h", _include("gatsspg.h"), _include("gatsspg_train.h"), _include("gatsspg_trainset.h")],
            tuning=True),
    Library("spp", ["spp_conv_kernels.hip", "spp_detect_kernels.hip", "spp_capi.hip"],
            ["spp_common.h", "gemm_f32_mfma.h", "gatsspg_common.h", "capi_common.h", "wg_primitives.h", _include("superpoint.h")], tuning=True),
    Library("pnp", ["pnp_kernels.hip"], ["capi_common.h", "geometry_math.h", "ransac_sample.h", "wg_primitives.h", _include("pnp.h"), _include("pnp_batch.h")]),
    Library("superglue", [os.path.join("superglue", "superglue.hip"), os.path.join("superglue", "nn_matcher.hip")],
            ["capi_common.h", "gemm_f32_mfma.h", "gatsspg_common.h", _include("superglue", "superglue.h"), _include("superglue", "nn_matcher.h")]),
    Library("det", [os.path.join("detector", "detector.hip"), os.path.join("detector", "flow.hip")],
            ["capi_common.h", "geometry_math.h", "ransac_sample.h", "wg_primitives.h", _include("detector", "detector.h"),
             _include("detector", "flow.h")]),
    Library("map", [os.path.join("mapping", "mapping.hip"), os.path.join("mapping", "bundle_adjust.hip"),
                    os.path.join("mapping", "track_update.hip")],
            ["capi_common.h", "geometry_math.h", "ransac_sample.h", "wg_primitives.h", _include("mapping", "mapping.h"),
             _include("mapping", "bundle_adjust.h"), _include("mapping", "track_update.h")]),
)
# views of the table under the names other modules use
LIB_PATH, SPP_LIB_PATH, PNP_LIB_PATH, SG_LIB_PATH, DET_LIB_PATH, MAP_LIB_PATH = (lib.path for lib in LIBRARIES)
SOURCES = LIBRARIES[0].sources
SG_SOURCES, SG_HEADERS = LIBRARIES[3].sources, LIBRARIES[3].headers
DET_SOURCES, DET_HEADERS = LIBRARIES[4].sources, LIBRARIES[4].headers
MAP_SOURCES, MAP_HEADERS = LIBRARIES[5].sources, LIBRARIES[5].headers


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _stale(lib, deps):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in (os.path.join(CSRC, s) for s in deps) if os.path.exists(d))


def is_stale():
    return any(_stale(lib.path, lib.sources + lib.headers) for lib in LIBRARIES)


def source_hash():
    """sha256 (first 16 hex digits) over the names and contents of every file under csrc/ and include/: identifies the build that a
    committed measurement (profiles/pmc_traffic.json) was taken on; bench.py says "stale" when it differs from the sources it runs."""
    import hashlib
    h = hashlib.sha256()
    for d in (CSRC, os.path.join(HERE, "..", "include")):
        for name in sorted(os.listdir(d)):
            if name.endswith((".hip", ".h")):
                h.update(name.encode())
                with open(os.path.join(d, name), "rb") as f:
                    h.update(f.read())
    return h.hexdigest()[:16]


def tuning_path(lib):
    return lib[:-3] + "_tuning.so"


def build(force=False, remarks=False, verbose=True, profiling=False, tuning=False, syntax_only=False):
    """Compile every HIP source for gfx950 into onepose_amd/lib/lib{gatsspg,spp,pnp,superglue,det,map}_hip.so.
    tuning / profiling builds go to lib*_tuning.so (environment knobs; profiling adds -DGATSSPG_PROFILING_BUILD: the timeline
    hooks) -- the package never loads those.  syntax_only: front-end check only."""
    os.makedirs(LIB_DIR, exist_ok=True)
    special = tuning or profiling
    for lib in LIBRARIES:
        if special and not lib.tuning:
            continue
        out = tuning_path(lib.path) if special else lib.path
        if not force and not syntax_only and not _stale(out, lib.sources + lib.headers):
            continue
        cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
        cmd += ["-fsyntax-only"] if syntax_only else ["-shared", "-o", out]
        if remarks:
            cmd.append("-Rpass-analysis=kernel-resource-usage")
        if special:
            cmd += ["-DGATSSPG_TUNING", "-DSPP_TUNING"]
        if profiling:
            cmd.append("-DGATSSPG_PROFILING_BUILD")
        cmd += [os.path.join(CSRC, s) for s in lib.sources]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=CSRC)
    return LIB_PATH


def asan_runtime():
    """Path of clang's shared AddressSanitizer runtime (LD_PRELOAD it into the python that loads an ASan build), or None."""
    import glob
    cands = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    return cands[-1] if cands else None


def build_asan(out_path):
    """Debug build of the matcher library with AddressSanitizer on the HOST side (argument checking, workspace carve-up, launch
    plumbing; device code is not instrumented): SURVEY.md section 5 'sanitizers'.  Never loaded by the package -- tests only."""
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-fsanitize=address", "-fno-gpu-sanitize",
           "-shared-libsan", "-o", out_path] + [os.path.join(CSRC, s) for s in SOURCES]
    subprocess.run(cmd, check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out_path


if __name__ == "__main__":
    build(force="--force" in sys.argv, remarks="--remarks" in sys.argv, profiling="--profiling" in sys.argv,
          tuning="--tuning" in sys.argv)
