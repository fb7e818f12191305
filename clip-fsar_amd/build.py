"""Build libclipfsar_hip.so, the side libraries (SIDE_LIBS), the extension libraries (EXT_LIBS), the add-on libraries (ADDON_LIBS) and the plug-in libraries (PLUGIN_LIBS) in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python clip-fsar_amd/build.py [--force]

The .so is git-ignored but travels to the GPU box with the gpurun snapshot.
"""
from __future__ import annotations

import collections
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libclipfsar_hip.so")
SOURCES = ["runtime.hip", "gemm.hip", "gemm_vit.hip", "frame_gemm.hip", "rowops.hip", "attention.hip", "tail.hip", "conv.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# Developer build (`python clip-fsar_amd/build.py --dev`): the same sources with -DCFSAR_DEV -- ablation switches and the
# cfsar_debug_* hooks of include/clipfsar_hip_dev.h -- as a SEPARATE library, libclipfsar_hip_dev.so, which clip_fsar_amd.hip
# loads only when CFSAR_DEV_LIB=1 (tools/*.py set it).  The product library contains none of it; tests/test_abi.py checks that.
DEV_LIB = os.path.join(HERE, "libclipfsar_hip_dev.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
         "-Rpass-analysis=kernel-resource-usage"]      # per-kernel VGPR / scratch report -> build/resource_usage.json
# Every source is compiled WITHOUT packed-fp32 VALU instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32).  Round 2: builds of the
# LN-folded GEMM that scaled accumulators with v_pk_mul_f32 occasionally returned stale values in lanes 48-63 of the HIGH register of one
# packed pair (once per ~100 launches, more often with a second kernel on the chip; docs/history/design_r01-r03.md "A fault worth recording").  Neither the
# round-2 microtests nor round 3's tools/ubench/pk_trans_waw.hip (transcendental -> packed WAW / RAW under a transcendental- or
# MFMA-heavy partner wave) reproduce it, so it is FENCED, not explained: with scalar fp32 VALU code it has not been seen (0 of 1 500
# stress launches against 44 of 150), and the fence now covers gemm.hip, attention.hip, tail.hip, conv.hip and rowops.hip as well (the same
# epilogue patterns live there).  Round 4 found one mechanism of this class -- the compiler spilling / reusing the destination of an inline-asm
# load before its data had landed, in exactly such a packed build -- and made those loads compiler-visible (profiles/r04_fault_audit.md);
# the fence stays because it costs nothing.  Same-box A/B: no measurable cost (profiles/r03_gemm_anatomy.md); MI355X_MICROARCH.md lists packed fp32
# beside MFMAs as an anti-lever anyway.  `-DCFSAR_PACKED_FP32` in CFSAR_BUILD_DEFS (developer builds) switches the instructions back on.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
SOURCE_FLAGS = {src: NO_PACKED_FP32 for src in SOURCES}
USAGE = os.path.join(HERE, "build", "resource_usage.json")
# Four tiers of libraries beside libclipfsar_hip.so; the first three are closed, the last one, PLUGIN_LIBS, is open.
# SIDE_LIBS, the side libraries, in the order they are built: the support gallery, its text half (EVAL_TEXT / COMBINE), the window streams'
# ring, gather and smoothing kernels, the same over the stream pool's descriptor table, frame ingest, the live gallery, grouped scoring, the
# last ViT block's class-token attention without its K | V projection, enrolment out of the stream pool's ring, and the text branches over
# grouped slot lists; C ABI of each in include/clipfsar_<name>.h.  Each is ONE source, csrc/<name>.hip, compiled with the product FLAGS and
# the fence into a library of its own beside libclipfsar_hip.so (the pinned export sets stay apart), stale when a file its source reaches
# through #include is newer, with its own resource report (build/resource_usage.json stays the product library's).  This tier is CLOSED:
# the table of tests/_abi.py and the staleness matrix of tests/test_build_recipe.py pin its ten names, every file of csrc/ and every
# include/clipfsar_*.h, so nothing is added to it and csrc/ takes no new file.
# EXT_LIBS (below build_side), the extension libraries, built after the side libraries by the same recipe -- one source, the same flags
# and fence, the same staleness rule, a resource report of its own -- from ext/<name>.hip with the C ABI in include/ext/clipfsar_<name>.h.
# This tier is closed as well: tests/test_class_smooth_abi.py pins its one name and the count of twelve libraries over both registries,
# so a further library cannot be a second name of EXT_LIBS.  It goes into ADDON_LIBS (below build_ext), the add-on libraries, built after
# the extensions by the same recipe again from ext/<name>.hip and include/ext/clipfsar_<name>.h: one more name there, its binding, and a
# test_<name>_abi.py with a _abi.Lib row of its own.  That tier closed in its turn: tests/test_events_abi.py pins its one name and the
# count of thirteen libraries over the three registries.  PLUGIN_LIBS (below build_addon), the plug-in libraries, built after the add-ons
# by the same recipe once more, is the LAST registry and stays OPEN: a further library is one more name there, ext/<name>.hip,
# include/ext/clipfsar_<name>.h, its binding and a test_<name>_abi.py with a _abi.Lib row of its own -- and such a test asserts that its
# name is in the registry and follows the recipe, never the registry's length or a total count of libraries.  An extension's, add-on's
# or plug-in's source may include csrc/ headers and headers of ext/ (the shared code keeps its one copy); nothing of csrc/ includes one
# of them.
# When a library is loaded is its binding's business, not the build's.
SideLib = collections.namedtuple("SideLib", "source lib usage")
SIDE_LIBS = {name: SideLib(name + ".hip", os.path.join(HERE, "libclipfsar_%s.so" % name),
                           os.path.join(HERE, "build", name, "resource_usage.json"))
             for name in ("gallery", "gallery_text", "stream", "pool", "ingest", "live", "groups", "lastblock", "enroll", "live_text")}


def side_lib_names() -> list:
    return list(SIDE_LIBS)


def _parse_usage(text: str) -> dict:
    """hipcc -Rpass-analysis=kernel-resource-usage remarks -> {mangled kernel name: {vgprs, agprs, scratch, spills, occupancy}}"""
    import re
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("agprs", r"remark:\s+AGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("spills", r"VGPRs Spill: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return out


def _includes(path, seen=None) -> set:
    """the files a source reaches through #include "..." (csrc headers and the public headers of include/), itself included"""
    import re
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path not in seen:
        seen.add(path)
        for inc in re.findall(r'^#include "([^"]+)"', open(path).read(), flags=re.M):
            _includes(os.path.join(os.path.dirname(path), inc), seen)
    return seen


def _side_deps(name) -> list:
    return sorted(_includes(os.path.join(CSRC, SIDE_LIBS[name].source))) + [os.path.abspath(__file__)]


def _product_deps() -> list:
    """every file of csrc/ that is not a side library's source or a header only side libraries include"""
    ours = set().union(*(_includes(os.path.join(CSRC, s)) for s in SOURCES))
    side_only = set().union(*(_includes(os.path.join(CSRC, sl.source)) for sl in SIDE_LIBS.values())) - ours
    return [p for p in (os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))) if p not in side_only] + [
        os.path.join(os.path.dirname(HERE), "include", "clipfsar_hip.h"), os.path.abspath(__file__)]


def _stale(lib, deps) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in deps)


# `python clip-fsar_amd/build.py --packed`: the PRODUCT sources and flags minus the fence, i.e. WITH packed-fp32 VALU instructions, as
# libclipfsar_hip_packed.so -- the build in which tools/asm_load_audit.py finds a compiler spill of a hidden load's destination before its
# wait (profiles/r04_fault_audit.md).  Loaded only through CFSAR_LIB_PATH (clip_fsar_amd.hip); exists to reproduce that finding on hardware.
PACKED_LIB = os.path.join(HERE, "libclipfsar_hip_packed.so")


def _compile(src, obj, extra, verbose) -> dict:
    """hipcc -c one source (a name of csrc/, or an absolute path) with FLAGS + extra; the resource-usage remarks come back parsed, the compiler's other output is printed"""
    cmd = [HIPCC] + FLAGS + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s" % (src, p.stdout))
    rest = "\n".join(l for l in p.stdout.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in l)
    if verbose and rest.strip():
        print(rest)
    return _parse_usage(p.stdout)


def _link(lib, objs, usage, usage_path, verbose) -> str:
    import json
    with open(usage_path, "w") as f:
        json.dump(usage, f, indent=0, sort_keys=True)
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib


def build_side(name, force: bool = False, verbose: bool = True) -> str:
    """a side library (a name of SIDE_LIBS): its one source -> its own library with the product FLAGS and the packed-fp32 fence,
    resource report -> .usage"""
    sl = SIDE_LIBS[name]
    if not force and not _stale(sl.lib, _side_deps(name)):
        return sl.lib
    bdir = os.path.dirname(sl.usage)
    os.makedirs(bdir, exist_ok=True)
    obj = os.path.join(bdir, sl.source.replace(".hip", ".o"))
    return _link(sl.lib, [obj], _compile(sl.source, obj, NO_PACKED_FP32, verbose), sl.usage, verbose)


# The extension tier (the comment above SIDE_LIBS): per-class smoothing of the stream pool.  A namedtuple type of its own, so that the
# side libraries' registry stays the only dict of SideLib values.
ExtLib = collections.namedtuple("ExtLib", "source header lib usage")
EXT = os.path.join(HERE, "ext")
EXT_LIBS = {name: ExtLib(os.path.join(EXT, name + ".hip"), os.path.join(os.path.dirname(HERE), "include", "ext", "clipfsar_%s.h" % name),
                         os.path.join(HERE, "libclipfsar_%s.so" % name), os.path.join(HERE, "build", name, "resource_usage.json"))
            for name in ("class_smooth",)}


def ext_lib_names() -> list:
    return list(EXT_LIBS)


def _ext_deps(name) -> list:
    return sorted(_includes(EXT_LIBS[name].source)) + [os.path.abspath(__file__)]


def _build_ext_lib(name, el, deps, force, verbose) -> str:
    """build_side's recipe on one ExtLib -- the product FLAGS, the packed-fp32 fence, stale when a file the source reaches through
    #include (or this file) is newer, resource report -> .usage"""
    if not force and not _stale(el.lib, deps):
        return el.lib
    bdir = os.path.dirname(el.usage)
    os.makedirs(bdir, exist_ok=True)
    obj = os.path.join(bdir, name + ".o")
    return _link(el.lib, [obj], _compile(el.source, obj, NO_PACKED_FP32, verbose), el.usage, verbose)


def build_ext(name, force: bool = False, verbose: bool = True) -> str:
    """an extension library (a name of EXT_LIBS): build_side's recipe on ext/<name>.hip"""
    return _build_ext_lib(name, EXT_LIBS[name], _ext_deps(name), force, verbose)


# The add-on tier (the comment above SIDE_LIBS): stream events, the detector of the stream pool.  ExtLib values in a registry of their own.
ADDON_LIBS = {name: ExtLib(os.path.join(EXT, name + ".hip"), os.path.join(os.path.dirname(HERE), "include", "ext", "clipfsar_%s.h" % name),
                           os.path.join(HERE, "libclipfsar_%s.so" % name), os.path.join(HERE, "build", name, "resource_usage.json"))
              for name in ("events",)}


def addon_lib_names() -> list:
    return list(ADDON_LIBS)


def _addon_deps(name) -> list:
    return sorted(_includes(ADDON_LIBS[name].source)) + [os.path.abspath(__file__)]


def build_addon(name, force: bool = False, verbose: bool = True) -> str:
    """an add-on library (a name of ADDON_LIBS): build_ext's recipe, after the extensions"""
    return _build_ext_lib(name, ADDON_LIBS[name], _addon_deps(name), force, verbose)


# The plug-in tier (the comment above SIDE_LIBS): adaptive baselines of the stream pool, the coarse stage of two-stage scoring
# (clip_fsar_amd.shortlist), the pinned selection of a stream pool with a shortlist, and the OTAM soft alignment behind a score
# (clip_fsar_amd.align), the tempo windows of a stream pool with rates=, and event evidence (clip_fsar_amd.evidence): an event's
# window copied out of the ring into a device store by the push that detected it, and the still-frame gate of a stream pool with
# still= (clip_fsar_amd.still): frames that did not change skip the tower, and the contest of a stream pool with contest=
# (clip_fsar_amd.contest): only a window's leading classes reach the detector, and the history search of a stream pool with history=
# (clip_fsar_amd.history): a class's best non-overlapping occurrences in the windows a store that outlives the ring still holds, and
# the shot ledger of a live gallery with ledger= (clip_fsar_amd.ledger): every shot's addend kept, so that shots leave, move and are audited,
# and the timeline of a stream pool with timeline= (clip_fsar_amd.timeline): every push's class scores folded into buckets of windows
# -- peak, its window, a count above a level -- that outlive the ring.
# ExtLib values again; the open registry.
PLUGIN_LIBS = {name: ExtLib(os.path.join(EXT, name + ".hip"), os.path.join(os.path.dirname(HERE), "include", "ext", "clipfsar_%s.h" % name),
                            os.path.join(HERE, "libclipfsar_%s.so" % name), os.path.join(HERE, "build", name, "resource_usage.json"))
               for name in ("baseline", "shortlist", "pool_select", "align", "tempo", "evidence", "still", "contest", "history", "ledger", "timeline")}


def plugin_lib_names() -> list:
    return list(PLUGIN_LIBS)


def _plugin_deps(name) -> list:
    return sorted(_includes(PLUGIN_LIBS[name].source)) + [os.path.abspath(__file__)]


def build_plugin(name, force: bool = False, verbose: bool = True) -> str:
    """a plug-in library (a name of PLUGIN_LIBS): build_ext's recipe, after the add-ons"""
    return _build_ext_lib(name, PLUGIN_LIBS[name], _plugin_deps(name), force, verbose)


def build(force: bool = False, verbose: bool = True, dev: bool = False, packed: bool = False, variant: str = "", defs=()) -> str:
    """variant / defs (developer A/B): the product build with extra -D flags as libclipfsar_hip_<variant>.so (loaded through CFSAR_LIB_PATH).
    The product build also builds the side libraries (build_side), after them the extension libraries (build_ext), then the add-on
    libraries (build_addon) and last the plug-in libraries (build_plugin)."""
    if not (dev or packed or variant):
        for name in side_lib_names():
            build_side(name, force=force, verbose=verbose)
        for name in ext_lib_names():
            build_ext(name, force=force, verbose=verbose)
        for name in addon_lib_names():
            build_addon(name, force=force, verbose=verbose)
        for name in plugin_lib_names():
            build_plugin(name, force=force, verbose=verbose)
    LIB_OUT = os.path.join(HERE, "libclipfsar_hip_%s.so" % variant) if variant else (PACKED_LIB if packed else (DEV_LIB if dev else LIB))
    if not force and not _stale(LIB_OUT, _product_deps()):
        return LIB_OUT
    bdir = os.path.join(HERE, "build", variant or "packed") if (packed or variant) else (os.path.join(HERE, "build", "dev") if dev else os.path.join(HERE, "build"))
    os.makedirs(bdir, exist_ok=True)
    extra = (os.environ.get("CFSAR_BUILD_DEFS", "").split() if dev else []) + list(defs)          # developer A/B builds only
    fenced = not (packed or "-DCFSAR_PACKED_FP32" in extra)                         # A/B: compile with the packed instructions
    extra = (["-DCFSAR_DEV"] if dev else []) + [e for e in extra if e != "-DCFSAR_PACKED_FP32"]
    objs = [os.path.join(bdir, src.replace(".hip", ".o")) for src in SOURCES]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(SOURCES)) as pool:                                  # every source at once: gemm.hip alone is most of the wall time
        reports = list(pool.map(lambda so: _compile(so[0], so[1], extra + (SOURCE_FLAGS.get(so[0], []) if fenced else []), verbose),
                                zip(SOURCES, objs)))
    usage = {}
    for r in reports:
        usage.update(r)
    return _link(LIB_OUT, objs, usage, USAGE if not (dev or packed or variant) else os.path.join(bdir, "resource_usage.json"), verbose)


if __name__ == "__main__":
    _v = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else ""
    _d = [a for a in sys.argv[1:] if a.startswith("-D")]
    print(build(force="--force" in sys.argv, dev="--dev" in sys.argv, packed="--packed" in sys.argv, variant=_v, defs=_d))
