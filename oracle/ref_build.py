"""ORACLE — test infrastructure only.  Build recipe for the reference's own
per-thread kernels as a host library, oracle/_ref/libref_kernels.so.

The kernel text is never copied into this repository.  At build time it is
cut out of the reference tree (S3_REFERENCE_DIR, default /root/reference)
into oracle/_ref/ (ignored by git), by function-name anchors:

  splatt3r_slam/backend/src/matching_kernels.cu
      everything except the #include lines and the two host launchers
      (refine_matches_cuda, iter_proj_cuda)  -> ref_matching_cut.inc
  splatt3r_slam/backend/src/gn_kernels.cu
      the EPS define, and the span after create_inds up to (not including)
      point_align_kernel: huber .. retrSim3, pose_retr_kernel
                                              -> ref_gn_cut.inc

and compiled by g++ together with our own driver (oracle/ref_shim/) under the
oracle Makefile's floating-point discipline.  Without the reference tree
nothing is built and nothing in oracle/_ref/ is touched.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "ref_shim")
OUT = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT, "libref_kernels.so")
SRC_DIR = os.path.join("splatt3r_slam", "backend", "src")
CXXFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
            "-Wno-unknown-pragmas", "-Wno-unused-label"]


def reference_dir() -> str:
    return os.environ.get("S3_REFERENCE_DIR", "/root/reference")


def _sources(ref):
    return [os.path.join(ref, SRC_DIR, f) for f in ("matching_kernels.cu", "gn_kernels.cu")]


def _anchor(lines, name, path):
    """Index of the line that opens the definition of function `name`."""
    pat = re.compile(r"\b%s\s*\(" % re.escape(name))
    hits = [i for i, l in enumerate(lines)
            if pat.search(l) and not l.lstrip().startswith("//") and "<<<" not in l]
    # a definition, not a call: no statement ends on that line
    hits = [i for i in hits if not lines[i].rstrip().endswith(";")]
    if not hits:
        raise RuntimeError(f"ref_build: anchor '{name}' not found in {path}")
    return hits[0]


def _def_start(lines, i):
    """Walk back from the anchor line over the definition's own leading lines
    (return type / qualifiers / template header on lines of their own)."""
    while i > 0:
        prev = lines[i - 1].strip()
        if not prev or prev.endswith(("}", ";")) or prev.startswith(("#", "//")):
            break
        i -= 1
    return i


def _def_end(lines, i, name, path):
    """Index of the line holding the closing brace of the definition at i."""
    depth, seen = 0, False
    for j in range(i, len(lines)):
        code = lines[j].split("//")[0]
        for ch in code:
            if ch == "{":
                depth += 1
                seen = True
            elif ch == "}":
                depth -= 1
                if seen and depth == 0:
                    return j
    raise RuntimeError(f"ref_build: no closing brace for '{name}' in {path}")


def cut_matching(path) -> str:
    lines = open(path).read().split("\n")
    drop = set(i for i, l in enumerate(lines) if l.lstrip().startswith("#include"))
    for name in ("refine_matches_cuda", "iter_proj_cuda"):
        a = _anchor(lines, name, path)
        drop.update(range(_def_start(lines, a), _def_end(lines, a, name, path) + 1))
    for name in ("refine_matches_kernel", "iter_proj_kernel"):
        if _anchor(lines, name, path) in drop:
            raise RuntimeError(f"ref_build: kernel '{name}' fell into a removed span")
    return "\n".join(l for i, l in enumerate(lines) if i not in drop) + "\n"


def cut_gn(path) -> str:
    lines = open(path).read().split("\n")
    eps = [l for l in lines if re.match(r"\s*#\s*define\s+EPS\b", l)]
    if len(eps) != 1:
        raise RuntimeError(f"ref_build: expected one EPS define in {path}, found {len(eps)}")
    a = _anchor(lines, "create_inds", path)
    lo = _def_end(lines, a, "create_inds", path) + 1
    hi = _def_start(lines, _anchor(lines, "point_align_kernel", path))
    if not lo < hi:
        raise RuntimeError(f"ref_build: create_inds does not precede point_align_kernel in {path}")
    body = lines[lo:hi]
    for name in ("huber", "quat_comp", "actSim3", "relSim3", "apply_Sim3_adj_inv", "expSO3",
                 "expSim3", "retrSim3", "pose_retr_kernel"):
        _anchor(body, name, path + " (cut span)")
    for bad in ("__shared__", "__syncthreads", "__shfl"):
        if any(bad in l.split("//")[0] for l in body):
            raise RuntimeError(f"ref_build: the cut span of {path} uses {bad}: not per-thread code")
    return "\n".join(eps + body) + "\n"


def _torch_include() -> str:
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    if not os.path.exists(os.path.join(inc, "c10", "util", "Half.h")):
        raise RuntimeError(f"ref_build: c10/util/Half.h not found under {inc}")
    return inc


def _stale(ref) -> bool:
    if not os.path.exists(LIB):
        return True
    deps = _sources(ref) + [os.path.abspath(__file__)] + \
        [os.path.join(SHIM, f) for f in os.listdir(SHIM)]
    return any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps)


def build(force: bool = False):
    """Build oracle/_ref/libref_kernels.so if the reference tree is present.
    Returns the library path, or None when there is no reference tree."""
    ref = reference_dir()
    if not (os.path.isdir(ref) and os.access(ref, os.R_OK | os.X_OK)):
        return None
    m_path, g_path = _sources(ref)
    for p in (m_path, g_path):
        if not os.path.isfile(p):
            raise RuntimeError(f"ref_build: reference tree at {ref} lacks {p}")
    if not force and not _stale(ref):
        return LIB
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        raise RuntimeError("ref_build: g++ not found")
    os.makedirs(OUT, exist_ok=True)
    for name, text in (("ref_matching_cut.inc", cut_matching(m_path)),
                       ("ref_gn_cut.inc", cut_gn(g_path))):
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)
    tmp = LIB + ".tmp"
    cmd = [cxx, *CXXFLAGS, "-shared", "-I", SHIM, "-I", OUT, "-I", _torch_include(),
           os.path.join(SHIM, "ref_driver.cpp"), "-o", tmp, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"ref_build: {' '.join(cmd)} failed:\n{r.stdout}\n{r.stderr}")
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force=True))
