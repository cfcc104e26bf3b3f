"""Build librgcn.so (hand-written HIP for gfx950) in-tree.

    python -m relationprediction_amd.build [--force] [--verbose]

hipcc cross-compiles without a GPU.  Objects go to build/, the library to
relationprediction_amd/lib/librgcn.so (git-ignored, but it travels to the GPU box).
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJDIR = os.path.join(ROOT, "build", "obj")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "librgcn.so")
# the same sources with -DRGCN_DEVTOOLS: adds the stand-alone GEMM entry points of include/rgcn_devtools.h for
# tools/ and the dense-contraction tests; the product library has none of them
LIB_DEVTOOLS = os.path.join(LIBDIR, "librgcn_devtools.so")
ARCH = "gfx950"
SOURCES = ["rgcn_api.hip", "rgcn_schedule.hip", "rgcn_devtools.hip", "graph_prep.hip", "csr_sort.hip", "gemm_f32.hip", "gemm_bf16x3.hip", "gemm_bf16x3_w8.hip", "block_msgs.hip", "block_rows.hip", "basis.hip", "basis_onehot.hip", "basis_tdiag.hip", "basis_pdiag.hip",
           "elementwise.hip", "highway.hip", "output_transform.hip", "decoder.hip", "adversarial.hip", "optimizer.hip", "ranking.hip", "relation_softmax.hip", "entity_softmax.hip", "sampler.hip", "neighborhood.hip", "comm.hip"]
HEADERS = [os.path.join(CSRC, "rgcn_internal.h"), os.path.join(CSRC, "rgcn_api_internal.h"), os.path.join(CSRC, "gemm_split.h"), os.path.join(CSRC, "gemm_plan.h"),
           os.path.join(CSRC, "dev_pool.h"), os.path.join(CSRC, "config_check.h"), os.path.join(CSRC, "optimizer_check.h"),
           os.path.join(CSRC, "row_walk.h"), os.path.join(CSRC, "counter_rng.h"), os.path.join(CSRC, "negative_exclusive.h"), os.path.join(CSRC, "negative_relation.h"), os.path.join(CSRC, "negative_reciprocal.h"),
           os.path.join(CSRC, "known_positives_index.h"), os.path.join(CSRC, "negative_typed.h"), os.path.join(CSRC, "type_sets.h"), os.path.join(CSRC, "pair_query.h"), os.path.join(CSRC, "relation_softmax_plan.h"),
           os.path.join(CSRC, "entity_softmax_plan.h"), os.path.join(CSRC, "entity_softmax_range.h"), os.path.join(CSRC, "adversarial_weights.h"),
           os.path.join(ROOT, "include", "rgcn.h"),
           os.path.join(ROOT, "include", "rgcn_devtools.h")]
DEVTOOLS_SOURCES = ["rgcn_api.hip", "rgcn_schedule.hip", "rgcn_devtools.hip", "comm.hip", "decoder.hip", "gemm_f32.hip"]       # the translation units the flag changes (knob())
# No packed-FP32 VALU instructions anywhere in the library: on gfx950 a v_pk_fma_f32 (and kin) issued
# by a wave that shares a CU with waves issuing v_mfma_f32_32x32x16_bf16 returns wrong low halves
# (reproducer: tools/mfma_corun.hip).  The encoder runs its HBM-bound kernels on side
# streams beside the bf16-split GEMM, so the feature is switched off for the device compile (the host
# pass prints "not a recognized feature" and ignores it) and the linked code objects are checked.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# -fvisibility=hidden: the library exports the C ABI of include/rgcn.h (whose declarations carry default visibility) and
# nothing else -- none of the C++ internals (tests/test_abi.py checks the dynamic symbol table)
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall",
         "-Wno-unused-function"] + NO_PACKED_FP32


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the R-GCN HIP library cannot be built")


def _digest(paths):
    h = hashlib.sha256()
    h.update(" ".join(FLAGS).encode())
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _llvm_objdump():
    for cand in ("/opt/rocm/lib/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")):
        if cand and os.path.exists(cand):
            return cand
    return None


def check_no_packed_fp32(lib=None):
    """Disassemble the gfx950 code objects of the library; raise if any packed-FP32 arithmetic is in them."""
    import glob
    import re
    import tempfile
    lib = lib or LIB
    objdump = _llvm_objdump()
    if objdump is None:
        raise RuntimeError("llvm-objdump not found: cannot verify the library is free of packed-FP32 ops")
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        subprocess.run([objdump, "--offloading", copy], capture_output=True, text=True, cwd=tmp, check=True)
        bad = []
        objs = glob.glob(copy + ".*amdgcn*")
        if not objs:
            raise RuntimeError("no device code objects found in " + lib)
        for co in objs:
            r = subprocess.run([objdump, "-d", co], capture_output=True, text=True, check=True)
            bad += re.findall(r"v_pk_(?:fma|mul|add)_f32", r.stdout)
        if bad:
            raise RuntimeError("librgcn.so contains %d packed-FP32 instructions (%s): they are unsafe beside the "
                               "bf16-split GEMM" % (len(bad), ", ".join(sorted(set(bad)))))
    return True


def build(force=False, verbose=False):
    os.makedirs(OBJDIR, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = _hipcc()
    jobs = []
    for src in SOURCES + [d + "@devtools" for d in DEVTOOLS_SOURCES]:
        dev = src.endswith("@devtools")
        src = src.replace("@devtools", "")
        sp = os.path.join(CSRC, src)
        obj = os.path.join(OBJDIR, src.replace(".hip", ".devtools.o" if dev else ".o"))
        stamp = obj + ".sha"
        dig = _digest([sp] + HEADERS) + ("+devtools" if dev else "")
        fresh = (not force and os.path.exists(obj) and os.path.exists(stamp)
                 and open(stamp).read() == dig)
        jobs.append((sp, obj, stamp, dig, fresh, dev))

    def compile_one(job):
        sp, obj, stamp, dig, fresh, dev = job
        if fresh:
            return None
        cmd = [hipcc] + FLAGS + (["-DRGCN_DEVTOOLS"] if dev else []) + ["-c", sp, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (sp, r.stderr[-4000:]))
        with open(stamp, "w") as f:
            f.write(dig)
        return r.stderr if verbose else None

    with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        outs = list(ex.map(compile_one, jobs))
    for o in outs:
        if o:
            sys.stderr.write(o)
    product = [j for j in jobs if not j[5]]
    devobj = {os.path.basename(j[0]): j[1] for j in jobs if j[5]}
    stale = any(not j[4] for j in jobs)
    for lib, objs in ((LIB, [j[1] for j in product]),
                      (LIB_DEVTOOLS, [devobj.get(os.path.basename(j[0]), j[1]) for j in product])):
        if force or stale or not os.path.exists(lib):
            # version script: whatever weak template instantiations the objects still carry (std::vector members ...)
            # stay local -- the dynamic symbol table is the C ABI alone
            vs = os.path.join(OBJDIR, "exports.map")
            with open(vs, "w") as f:
                f.write("{ global: rgcn_*; local: *; };\n")
            cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-Wl,--version-script=" + vs, "-o", lib] + objs + ["-ldl"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("link failed:\n" + r.stderr[-4000:])
            check_no_packed_fp32(lib)
    return LIB


def build_test_collective(force=False, device_side=False):
    """tests/collective_double/shm_collective.hip -> its _build/libshmcollective.so: the shared-memory stand-in
    for librccl that tests/test_gpu_multiprocess.py binds through RGCN_RCCL_LIBRARY (test infrastructure; host
    code only, compiled here so that the prebuilt .so travels to the GPU box with the tree).  device_side=True:
    ipc_collective.hip -> libipccollective.so, the stand-in whose collectives are kernels (capturable)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "ipc_collective" if device_side else "shm_collective"
    src = os.path.join(root, "tests", "collective_double", name + ".hip")
    outdir = os.path.join(root, "tests", "collective_double", "_build")
    out = os.path.join(outdir, "lib%s.so" % name.replace("_", ""))
    stamp = out + ".sha"
    dig = _digest([src])
    if not force and os.path.exists(out) and os.path.exists(stamp) and open(stamp).read() == dig:
        return out
    os.makedirs(outdir, exist_ok=True)
    r = subprocess.run([_hipcc(), "--offload-arch=" + ARCH, "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out,
                        "-lrt"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
    with open(stamp, "w") as f:
        f.write(dig)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
