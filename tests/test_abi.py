"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/rgcn.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from relationprediction_amd import build
    return build.build()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rgcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rgcn_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for must in ["rgcn_create", "rgcn_destroy", "rgcn_set_graph", "rgcn_forward", "rgcn_backward",
                 "rgcn_get_grad", "rgcn_set_param", "rgcn_comm_init", "rgcn_last_error"]:
        assert must in syms


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for s in declared_symbols():
        assert hasattr(lib, s), "librgcn.so does not export %s" % s
    lib.rgcn_abi_version.restype = ctypes.c_int32
    assert lib.rgcn_abi_version() == 1


def _dynamic_symbols(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in "TtDdBbRrWwVv")


def test_library_exports_nothing_but_the_header(lib_path):
    """-fvisibility=hidden + default visibility on include/rgcn.h's declarations: the dynamic symbol table of
    librgcn.so is the header's names and NOTHING else (round 3 exported 63 mangled C++ internals beside them); the
    devtools build adds include/rgcn_devtools.h's names only.  The collective-library override (RGCN_RCCL_LIBRARY) is a
    seam of the devtools build: the product library does not even contain the string."""
    from relationprediction_amd import build
    ignore = {"_init", "_fini", "__bss_start", "_edata", "_end", "__hip_fatbin", "__hip_fatbin_wrapper"}
    got = [x for x in _dynamic_symbols(lib_path) if x not in ignore and not x.startswith("__hip_")]
    assert got == declared_symbols(), sorted(set(got) ^ set(declared_symbols()))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgcn_devtools.h")).read(), flags=re.S)
    dev = set(re.findall(r"\b(rgcn_[a-z_0-9]+)\s*\(", text))
    got_dev = [x for x in _dynamic_symbols(build.LIB_DEVTOOLS) if x not in ignore and not x.startswith("__hip_")]
    assert got_dev == sorted(set(declared_symbols()) | dev), sorted(set(got_dev) ^ (set(declared_symbols()) | dev))
    assert b"RGCN_RCCL_LIBRARY" not in open(lib_path, "rb").read()
    assert b"RGCN_RCCL_LIBRARY" in open(build.LIB_DEVTOOLS, "rb").read()


def test_binding_matches_header(lib_path):
    from relationprediction_amd import _native
    assert _native.exported_symbols() == declared_symbols()
    _native.load_library()          # attaches prototypes; raises if a symbol is missing
    assert ctypes.sizeof(_native.RgcnConfig) == 64


def test_experiment_hooks_live_in_the_devtools_build_only(lib_path):
    """the product library exports nothing but include/rgcn.h; the stand-alone GEMM entry points of
    include/rgcn_devtools.h exist in librgcn_devtools.so (-DRGCN_DEVTOOLS) only, and no ablation switch is left in
    the product sources"""
    from relationprediction_amd import _native, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgcn_devtools.h")).read(), flags=re.S)
    dev = sorted(set(re.findall(r"\b(rgcn_[a-z_0-9]+)\s*\(", text)))
    assert dev == _native.exported_devtools_symbols() and dev
    product, devtools = ctypes.CDLL(lib_path), ctypes.CDLL(build.LIB_DEVTOOLS)
    for s in dev:
        assert not hasattr(product, s), "product library exports %s" % s
        assert hasattr(devtools, s)
    for s in declared_symbols():
        assert hasattr(devtools, s)
    for name in os.listdir(build.CSRC):
        src = open(os.path.join(build.CSRC, name)).read()
        assert "RGCN_GEMM_ABLATE" not in src and "ablate" not in src, name


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rgcn.h"\n#include "rgcn_devtools.h"\nint main(void){ rgcn_config c; (void)c; return sizeof(rgcn_config) == 64 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    import subprocess
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_no_gpu_means_loud_failure(lib_path):
    """Without a GPU the product path must raise, not fall back to anything."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present")
    from relationprediction_amd import _native
    with pytest.raises(_native.RgcnError):
        _native.Engine(16, 9, 10, 1, "block", 2, max_edges=50)


def test_device_info_is_context_free_and_reports_no_device_without_a_gpu(lib_path):
    """rgcn_device_info needs no context (bench.py --gpus N calls it before it creates one): without a GPU it reports zero
    devices and no PCI address, and NULL outputs are refused."""
    lib = ctypes.CDLL(lib_path)
    lib.rgcn_device_info.restype = ctypes.c_int32
    lib.rgcn_device_info.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    n, pci = ctypes.c_int32(-7), ctypes.c_int64(-7)
    assert lib.rgcn_device_info(0, None, ctypes.byref(pci)) == 1          # RGCN_ERR_INVALID
    assert lib.rgcn_device_info(0, ctypes.byref(n), ctypes.byref(pci)) == 0
    if os.path.exists("/dev/kfd"):
        assert n.value >= 1 and pci.value >= 0
        assert lib.rgcn_device_info(n.value, ctypes.byref(n), ctypes.byref(pci)) == 0 and pci.value == -1   # past the last one
    else:
        assert (n.value, pci.value) == (0, -1)
    from relationprediction_amd import _native
    count, address = _native.Engine.device_info(0)                           # the ctypes binding of the same call
    assert lib.rgcn_device_info(0, ctypes.byref(n), ctypes.byref(pci)) == 0 and (count, address) == (n.value, pci.value)


def test_library_has_no_packed_fp32_instructions():
    """gfx950: packed-FP32 VALU ops return wrong low halves beside waves that issue bf16 MFMAs
    (tools/mfma_corun.hip); the build switches the feature off and this checks the linked code objects."""
    from relationprediction_amd import build
    build.build()
    assert build.check_no_packed_fp32()


def test_bench_workloads_are_backed_by_fixtures_and_fail_loudly_without_a_gpu():
    """every bench.py workload names a graph in tests/golden/graphs.npz of the stated size and a legal geometry;
    on a box without a GPU the bench exits non-zero with the library's error instead of falling back to anything"""
    import importlib.util
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name, (graph, V, R, d, L, kind, nb, E) in bench.WORKLOADS.items():
        t = bench.load_graph(graph)        # a fixture of tests/golden/graphs.npz, or drawn from one's histograms
        assert t.shape == (E, 3) and t.dtype == np.int32, name
        assert t[:, [0, 2]].max() < V and t[:, 1].max() < R and t.min() >= 0, name
        if graph.startswith("synth:"):
            assert len(np.unique(t, axis=0)) == E, name
            assert np.array_equal(t, bench.load_graph(graph)), name      # deterministic
        if kind == "block":
            assert d % nb == 0 and d // nb in (1, 2, 3, 4, 5, 8), name
    assert set(bench.EXTRA_WORKLOADS) <= set(bench.WORKLOADS)
    if not os.path.exists("/dev/kfd"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--cpu-steps", "0"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "librgcn status" in r.stderr and not r.stdout.strip()


def test_bench_result_line_stays_compact_and_self_spawns():
    """bench.compact_line keeps the driver's line to a few KB whatever the per-kernel tables hold (round 2's 65 KB line
    could not be parsed by the driver), and `bench.py --gpus 2` without a launcher starts its own ranks (here, without a
    GPU, they fail loudly and the parent reports which)."""
    import importlib.util
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    kern = [{"kernel": "kernel_number_%d" % i, "launches_per_step": 2.0, "avg_us": 12.34, "avg_us_in_pipeline": 23.45,
             "ms_per_step": 0.0247, "bound": "hbm", "achieved": 4321.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.54,
             "compulsory_bytes": 1.2e8, "design_bytes": 1.9e8, "alg_flops": 0.0, "design_gbs": 5000.0, "traffic": 2.0e8}
            for i in range(40)]
    roof = dict(kern[0], traffic_source="profiles/x.json", basis="...")
    sr = {k: 1.0 for k in ("compulsory_bytes_per_step", "design_bytes_per_step", "pmc_bytes_per_step", "alg_flops_per_step",
                           "hbm_frac", "fp32_mfma_frac", "serial_ceiling_ms", "frac_of_serial_ceiling",
                           "sum_exclusive_kernel_ms")}
    wl = {"config": {"workload": "some_workload_name"}, "value": 1.0, "ms_per_step": 1.0, "roofline": roof,
          "step_roofline": sr, "kernels": kern}
    out = {"metric": "m" * 80, "value": 1.0, "unit": "edges/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 0.6,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32 " + "x" * 200,
           "data": "y" * 250, "config": {"workload": "fb237_block", "step": "z" * 200}, "roofline": roof,
           "step_roofline": sr, "kernels": kern, "workloads": [wl] * 6,
           "cpu_baseline": {"value": 1.0, "unit": "edges/s", "cores": 256, "kind": "port", "sample": "s" * 150,
                            "ms_per_step": 900.0, "threads": "t" * 300},
           "cpu_baseline_reference_code": bench.reference_code_baseline(),
           "train_steps": [{"workload": "w" * 24, "minibatch_step": {"ms_per_step": 1.2, "edges_per_s": 1e7, "kernels": kern},
                            "captured_step": {"ms_per_step_hipgraph_replay": 1.2, "ms_per_step_stream_launched": 1.2}}] * 2,
           "evaluation": {"graph_edges": 272115, "queries": 2000, "encode_full_graph_ms": 1.6, "rank_both_sides_ms": 2.5,
                          "ranked_triples_per_s": 8e5, "note": "n" * 300}, "details": "bench_details.json",
           "train_loop": {"ms_per_iteration": 1.5, "iterations_per_s": 666.0, "device_step_ms": 1.2,
                          "device_idle_frac": 0.2, "host_batch_build_ms": 5.0,
                          "ms_per_iteration_by_builder_threads": {"0": 6.0, "8": 1.5},
                          "ms_per_iteration_device_sampler": 1.3, "sampler": "s" * 100}}
    line = json.dumps(bench.compact_line(out), separators=(",", ":"))
    assert len(line) < 6000, len(line)
    assert out["cpu_baseline_reference_code"]["kind"] == "reference-code-over-torch-shim"
    if not os.path.exists("/dev/kfd"):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--cpu-steps", "0"],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode != 0 and "rank(s) failed" in r.stderr and "must be launched" not in r.stderr


def test_bench_dump_outputs_are_a_fixed_sample_within_64_mb(tmp_path):
    """bench.write_outputs: small arrays as they are, a larger one as the same seeded sample of DUMP_MAX_ENTRIES entries on
    every call, float32; more than 64 MB in all is refused before anything is written."""
    import importlib.util
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_MAX_ENTRIES
    big = np.arange(n + 5, dtype=np.float64)
    small = np.random.RandomState(0).randn(7, 3)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (n,) and np.array_equal(a, b)
    assert len(np.unique(a)) == n and np.all(np.diff(a) > 0)             # distinct positions, in order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.astype(np.float32))
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "c"), {"x%d" % i: big for i in range(9)})
    assert not (tmp_path / "c").exists()
