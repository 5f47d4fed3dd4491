"""Build libedtr_hip.so (gfx950) in-tree with hipcc.  `python -m edtr_amd.build` or build_library()."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "libedtr_hip.so")
SOURCES = ["igemm.hip", "halo512.hip", "attention.hip", "attn512.hip", "norm.hip", "elementwise.hip", "swin.hip", "ffn.hip", "lin320.hip", "rng.hip", "imageio.hip", "degrade.hip", "degrade2.hip", "labels.hip", "boxes.hip"]
# units that include glue.h and are newer than the glue / MFMA table tests/test_host_logic.py pins SOURCES to; compiled and linked alike
GLUE_SOURCES = ["coco.hip", "cls.hip", "rois.hip", "coco_acc.hip", "det_transform.hip", "targets.hip", "seg_loss.hip", "losses.hip"]
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
ABI_HEADER = os.path.join(INCLUDE, "edtr_hip.h")
ARCH = "gfx950"


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (needed to build libedtr_hip.so)")


_INCLUDE_LINE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+(?:"([^"]+)"|([A-Za-z_]\w*))', re.M)


def object_deps(src: str) -> list:
    """The files the object of csrc/``src`` is compiled from, the source first: its quoted #include lines followed through csrc/ and
    include/ (depth first, in the order of the lines, each file once), so that a header can never be forgotten in a hand-kept table.
    `#include NAME` takes the file of the `#define NAME "file"` next to it (a regenerated .inc must rebuild its object).  A quoted
    include that is no file of these two directories is an error; <system> headers belong to the toolchain."""
    deps: list = []

    def visit(path):
        path = os.path.normpath(path)
        if path in deps:
            return
        if os.path.dirname(path) not in (CSRC, INCLUDE) or not os.path.isfile(path):
            raise RuntimeError(f"{src}: #include of {path}, which is no file of csrc/ or include/")
        deps.append(path)
        with open(path) as fh:
            text = fh.read()
        for quoted, macro in _INCLUDE_LINE.findall(text):
            if macro:
                default = re.search(r'^[ \t]*#[ \t]*define[ \t]+%s[ \t]+"([^"]+)"' % macro, text, re.M)
                if not default:
                    raise RuntimeError(f"{os.path.basename(path)}: #include {macro} without a #define {macro} \"file\"")
                quoted = default.group(1)
            visit(os.path.join(os.path.dirname(path), quoted))

    visit(os.path.join(CSRC, src))
    return deps


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def source_hash() -> str:
    """sha1 over the kernel sources (csrc/*.hip, *.inc, *.h and the ABI header): stamps measurements that are read back later
    (bench.py refuses a committed PMC traffic figure measured on different kernel code; .git does not travel to the GPU box)."""
    import hashlib
    h = hashlib.sha1()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".inc", ".h")))
    for path in [os.path.join(CSRC, f) for f in files] + [ABI_HEADER]:
        with open(path, "rb") as fh:
            h.update(os.path.basename(path).encode() + b"\0" + fh.read())
    return h.hexdigest()[:12]


def _object_key(flags, deps) -> str:
    """sha1 over the compile flags and the bytes of every dependency: an object is reused only when this matches the key
    written next to it, so an object compiled elsewhere or with other -D flags can never be linked by accident (mtimes lie)."""
    import hashlib
    h = hashlib.sha1(" ".join(flags).encode())
    for d in deps:
        with open(d, "rb") as fh:
            h.update(b"\0" + os.path.basename(d).encode() + b"\0" + fh.read())
    return h.hexdigest()


def build_library(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    objs = []
    relink = force
    jobs = []
    for src in SOURCES + GLUE_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        # -Werror=pass-failed: a `#pragma unroll` the optimizer could not honour is an ERROR — in round 4 such a loop around the
        # shared epilogue silently stayed rolled and sent a kernel's accumulators through scratch memory
        flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Werror=pass-failed"]
        key = _object_key(flags, object_deps(src))
        keyfile = o + ".key"
        have = open(keyfile).read().strip() if os.path.exists(keyfile) and os.path.exists(o) else ""
        if force or have != key:
            jobs.append(([hipcc] + flags + ["-c", s, "-o", o], keyfile, key))
        objs.append(o)

    def _compile(job):
        cmd, keyfile, key = job
        if verbose:
            print(" ".join(cmd), flush=True)
        if os.path.exists(keyfile):
            os.remove(keyfile)                 # (a failed compile must not leave a key that vouches for the old object)
        subprocess.run(cmd, check=True)
        with open(keyfile, "w") as fh:
            fh.write(key + "\n")

    if jobs:
        # translation units compile independently: a few at a time (the container has 8 cores; one hipcc peaks near 3 GB)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), int(os.environ.get("EDTR_BUILD_JOBS", "4")))) as pool:
            list(pool.map(_compile, jobs))
        relink = True
    if relink or _stale(LIB_PATH, objs):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB_PATH


if __name__ == "__main__":
    if "--hash" in sys.argv:
        print(source_hash())
    else:
        print(build_library(force="--force" in sys.argv, verbose=True))
