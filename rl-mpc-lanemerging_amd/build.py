"""Build the gfx950 shared library (``libstmpc.so``) in-tree with hipcc.

The library is the product's only compute path; importing the package does not build
anything, and every solver entry fails loudly if the library or a GPU is missing.

The host code is three translation units (``UNITS``: the solver; the core with the context, the controllers, the episode world and
the vector env; the learners): each is compiled to an object under ``build/``, in parallel, and one link step makes the library.
Only the units whose sources changed are compiled again (and the core, which carries the ``src=`` stamp).
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
BUILD_DIR = os.path.join(PKG_DIR, "build")
LIB_PATH = os.path.join(PKG_DIR, "libstmpc.so")
STMPC_H = os.path.join(REPO_ROOT, "include", "stmpc.h")

# csrc/<unit>.hip, the longest compile first.  CORE_UNIT carries the src= stamp of stmpc_backend_info.
UNITS = ["stmpc_solver", "stmpc", "stmpc_learner"]
CORE_UNIT = "stmpc"

HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17",
    # bit-exactness with the reference: one IEEE op per source op, no reassociation
    "-ffp-contract=off", "-fno-fast-math",
    "-fPIC", "-shared",
]

LAST_BUILD = {"compiled": [], "linked": False}      # what the last build() call did (its log)


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def source_hash():
    """sha256[:16] over the library's sources (csrc/* and include/stmpc.h, by name).  Compiled into the library
    (``stmpc_backend_info`` ends with ``src=<hash>``) and stamped into profiles/*/measured.json, so that counters
    taken from another build of the kernels are recognisable as stale."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".h")))
    files.append(STMPC_H)
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    lib_m = os.path.getmtime(LIB_PATH)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [STMPC_H]
    return any(os.path.getmtime(s) > lib_m for s in srcs)


def unit_source(unit):
    return os.path.join(CSRC, unit + ".hip")


def unit_object(unit):
    return os.path.join(BUILD_DIR, unit + ".o")


def unit_deps(unit):
    """The files a unit is compiled from: its .hip, include/stmpc.h and the headers the compiler listed when it last built the unit
    (build/<unit>.d); None when there is no such list yet."""
    dep = os.path.join(BUILD_DIR, unit + ".d")
    if not os.path.exists(dep):
        return None
    words = open(dep).read().replace("\\\n", " ").split()
    files = {os.path.normpath(os.path.join(PKG_DIR, w)) for w in words[1:] if not w.endswith(":")}
    return sorted(files | {unit_source(unit), STMPC_H})


def stale_units(deps, mtimes, objects):
    """The units to compile again, as a pure function of modification times.  deps: unit -> the files it is compiled from (None: not known);
    mtimes: file -> modification time (a listed file that is gone counts as changed); objects: unit -> its object's modification time, None
    when there is none.  A unit is stale when it has no object or no file list, or one of its files is newer than its object; the core unit
    is also stale whenever another unit is, so that its src= stamp is the hash of the sources every object was built from."""
    def stale(u):
        if objects.get(u) is None or deps.get(u) is None:
            return True
        return any(mtimes.get(f) is None or mtimes[f] > objects[u] for f in deps[u])
    out = [u for u in deps if stale(u)]
    if out and CORE_UNIT in deps and CORE_UNIT not in out:
        out.append(CORE_UNIT)
    return out


def _mtime(path):
    return os.path.getmtime(path) if os.path.exists(path) else None


def _compile(hipcc, unit, src_hash, verbose):
    cmd = [hipcc] + [f for f in HIPCC_FLAGS if f != "-shared"] + ["-c"]
    if unit == CORE_UNIT:
        cmd.append('-DSTMPC_SRC_HASH="%s"' % src_hash)
    cmd += ["-I" + os.path.join(REPO_ROOT, "include"), "-MMD", "-MF", os.path.join(BUILD_DIR, unit + ".d"), unit_source(unit), "-o", unit_object(unit)]
    if verbose:
        print(" ".join(cmd), flush=True)
    return unit, subprocess.run(cmd, capture_output=True, text=True, cwd=PKG_DIR)


def build(force=False, verbose=False):
    """Compile the stale units of csrc/ for gfx950 and link ``libstmpc.so`` next to this file."""
    LAST_BUILD["compiled"], LAST_BUILD["linked"] = [], False
    if not force and not needs_build():
        return LIB_PATH
    os.makedirs(BUILD_DIR, exist_ok=True)
    deps = {u: unit_deps(u) for u in UNITS}
    mtimes = {f: _mtime(f) for fs in deps.values() if fs for f in fs}
    todo = list(UNITS) if force else stale_units(deps, mtimes, {u: _mtime(unit_object(u)) for u in UNITS})
    if not todo and not force:
        todo = [CORE_UNIT]      # a source no unit lists yet has changed (needs_build() looks at all of csrc/): the src= stamp follows source_hash()
    hipcc, src_hash = find_hipcc(), source_hash()
    if todo:
        workers = min(len(UNITS), int(os.environ.get("MAX_JOBS", 8)), 16)
        with ThreadPoolExecutor(max_workers=workers) as pool:
            results = list(pool.map(lambda u: _compile(hipcc, u, src_hash, verbose), todo))
        for unit, res in results:
            if res.returncode != 0:
                raise RuntimeError("hipcc failed on %s:\n%s%s" % (unit, res.stdout, res.stderr))
        LAST_BUILD["compiled"] = todo
    cmd = [hipcc] + HIPCC_FLAGS + [unit_object(u) for u in UNITS] + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed to link:\n" + res.stdout + res.stderr)
    LAST_BUILD["linked"] = True
    return LIB_PATH
