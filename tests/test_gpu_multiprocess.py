"""The multi-process paths on the one-GPU test box: several ranks as separate processes on ONE device, with the
shared-memory stand-in of tests/collective_double bound in place of librccl (RGCN_RCCL_LIBRARY; RCCL itself
refuses two ranks on one GPU).  Covers what the in-process phase-API tests cannot: the library's own
exchange call sites -- reduce-scatter of the partial rows, all-gather of the finished ones on a side stream, one
all-reduce of the replicated weight gradients -- (rgcn_step_device / rgcn_train_step_device on world > 1 contexts) and bench.py's whole
--gpus N control flow under the torch.distributed.run launcher."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLE = os.path.join(ROOT, "tests", "collective_double")


@pytest.fixture(scope="module")
def collective():
    from relationprediction_amd import build
    return build.build_test_collective()


def launch(nproc, port, script_args, collective, extra_env=None, timeout=240):
    env = dict(os.environ)
    env["RGCN_RCCL_LIBRARY"] = collective
    env["RGCN_LIBRARY"] = "devtools"        # the collective override is a seam of librgcn_devtools.so only
    env.update(extra_env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port)] + script_args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("world,kind,nb", [(2, "block", 8), (3, "block", 8), (4, "block", 8), (2, "basis", 2),
                                           (3, "basis", 2)])
def test_sharded_steps_across_processes(collective, world, kind, nb):
    r = launch(world, 29600 + world + (10 if kind == "basis" else 0),
               [os.path.join(DOUBLE, "sharded_worker.py"), kind, str(nb)], collective)
    assert r.returncode == 0, r.stdout[-2000:] + "\n".join(l for l in r.stderr.splitlines() if "elastic" not in l and "torch/distributed" not in l)[-4000:]
    assert "SHARDED-OK world=%d kind=%s" % (world, kind) in r.stdout


@pytest.fixture(scope="module")
def device_collective():
    from relationprediction_amd import build
    return build.build_test_collective(device_side=True)


@pytest.mark.parametrize("world,kind,nb", [(2, "block", 8), (3, "block", 8), (2, "basis", 2)])
def test_captured_sharded_train_step(device_collective, world, kind, nb):
    """BASELINE.json configs[4] as written -- a hipGraph-captured train step on a relation-sharded context -- with the
    collectives INSIDE the graph (the device-side stand-in of tests/collective_double/ipc_collective.hip: kernels and
    hipIpc mailboxes, no host synchronisation): replays equal the directly issued steps bitwise, on every rank."""
    r = launch(world, 29700 + world + (10 if kind == "basis" else 0),
               [os.path.join(DOUBLE, "captured_worker.py"), kind, str(nb)], device_collective,
               {"RGCN_CAPTURE_SHARDED": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + "\n".join(l for l in r.stderr.splitlines() if "elastic" not in l and "torch/distributed" not in l)[-4000:]
    assert "CAPTURED-SHARDED-OK world=%d kind=%s" % (world, kind) in r.stdout


def check_multi_rank_line(r, world):
    assert r.returncode == 0, r.stdout[-2000:] + "\n".join(l for l in r.stderr.splitlines() if "elastic" not in l and "torch/distributed" not in l)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines[-1]) < 8192                                 # the driver keeps an 8 KB tail: the line must fit
    out = json.loads(lines[-1])                                  # the JSON line is the LAST line on stdout
    assert sum(1 for l in lines if l.startswith("{")) == 1
    assert out["n_gpus"] == world and out["steps"] == 4 and out["value"] > 0
    assert out["config"]["parallelism"].startswith("relation-sharded x%d" % world)
    assert out["roofline"] and out["comm_ms_per_step"] > 0
    # what the collective library itself reports (ncclCommCount), and the collectives of one step by name
    assert out["rccl_ranks"] == world and {c[0] for c in out["collectives"]} >= {"rccl_reduce_scatter", "rccl_all_gather"}
    with open(os.path.join(ROOT, out["details"])) as f:          # the per-kernel tables live in the side file
        names = {k["kernel"] for k in json.load(f)["kernels"]}
    assert {"rccl_allreduce", "rccl_reduce_scatter", "rccl_all_gather"} <= names


@pytest.mark.parametrize("world", [2, 4])
def test_bench_multi_rank_prints_one_json_line_last(collective, world):
    r = launch(world, 29650 + world, ["bench.py", "--gpus", str(world), "--steps", "4", "--warmup", "1",
                                      "--cpu-steps", "0", "--full"], collective, {"RGCN_BENCH_SHARE_GPU": "1"})
    check_multi_rank_line(r, world)


def test_bench_refuses_ranks_that_share_a_gpu(collective):
    """Two ranks on a box whose launcher leaves them ONE visible device, without the tests' override: both take device 0
    (rgcn_device_info: one device visible), the communicator comes up, and the self-check -- PCI addresses gathered over
    the communicator -- ends the run with status 3 and says why, instead of printing a number that "scales" at 1/N."""
    r = launch(2, 29671, ["bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--cpu-steps", "0"], collective, {})
    assert r.returncode != 0
    assert "multi-GPU self-check FAILED" in r.stderr and "ranks share a device" in r.stderr, r.stderr[-3000:]
    assert not any(l.startswith("{") for l in r.stdout.splitlines())


@pytest.mark.parametrize("world", [2, 3])
def test_bench_spawns_its_own_ranks_without_a_launcher(collective, world):
    """`python3 bench.py --gpus N` as the driver calls it (no torch.distributed.run, no WORLD_SIZE): the script starts
    its N ranks itself and relays rank 0's line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(RGCN_RCCL_LIBRARY=collective, RGCN_LIBRARY="devtools", RGCN_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "4", "--warmup", "1",
                        "--cpu-steps", "0", "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    check_multi_rank_line(r, world)


def test_bench_single_gpu_line_carries_every_section():
    """The --full call with small counts: ONE compact JSON line (the last line of stdout, under 8 KB) with the contract
    keys, the roofline and cpu_baseline objects, one-line summaries of the other BASELINE configurations ("workloads"),
    the device train steps ("train_steps", config 5's captured step among them) and the evaluation pass ("evaluation");
    the per-kernel tables in bench_details.json."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--extra-steps", "2",
                        "--cpu-steps", "1", "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines[-1]) < 8192, len(lines[-1])
    d = json.loads(lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["config"]["workload"] == "fb237_block" and d["value"] > 0
    assert d["config"]["norm_mode"].startswith("intended")
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "compulsory_bytes", "design_bytes"} <= set(d["roofline"])
    assert 0 < d["roofline"]["frac"] <= 1
    # HBM bytes per launch: measured in this run (two rocprofv3 --pmc passes of the script itself), or -- when rocprofv3
    # is missing or a pass fails -- the committed figures
    src = d["roofline"]["traffic_source"]
    assert d["roofline"]["traffic"] > 0 and (src.startswith("measured in this run") or src.startswith("profiles/")), src
    assert {"value", "unit", "cores", "kind", "sample"} <= set(d["cpu_baseline"])
    assert d["cpu_baseline_reference_code"]["kind"].startswith("reference-code") \
        and d["cpu_baseline_reference_code"]["measured_in_this_run"] is False
    assert [w["workload"] for w in d["workloads"]] == ["fb237_basis_b2", "fb237_basis_b5", "wn18_block", "fb15k_block",
                                                       "fb237_block_fullgraph", "fb237_block_traingraph"]
    assert all(w["ms_per_step"] > 0 and w["kernel"] and 0 < w["frac"] <= 1 for w in d["workloads"])
    assert [t["workload"] for t in d["train_steps"]] == ["fb237_block_train_step", "fb15k_block_train_step"]
    for t in d["train_steps"]:
        assert t["ms_per_step"] > 0 and t["hipgraph_ms"] > 0 and t["stream_ms"] > 0 and t["top"]
    assert d["evaluation"]["ranked_triples_per_s"] > 0 and d["evaluation"]["encode_full_graph_ms"] > 0
    tl = d["train_loop"]           # the whole iteration through the driver: host sampler + upload + device step + loss
    # (the loop now runs within 2 % of the device step, and this call times the step over TWO launches: no order between
    # the two numbers is asserted)
    assert tl["ms_per_iteration"] > 0 and tl["device_step_ms"] > 0 and 0 <= tl["device_idle_frac"] < 1
    assert set(tl["ms_per_iteration_by_builder_threads"]) == {"0", "8"} and tl["ms_per_iteration_device_sampler"] > 0
    with open(os.path.join(ROOT, d["details"])) as f:
        full = json.load(f)
    # no kernel of any workload or train step claims more than its roofline
    tables = [full["kernels"]] + [w["kernels"] for w in full["workloads"]] + \
             [t["minibatch_step"]["kernels"] for t in full["train_steps"]]
    assert all(k["frac"] <= 1.0 for tab in tables for k in tab), [k for tab in tables for k in tab if k["frac"] > 1.0]
    assert all({"compulsory_bytes", "design_bytes", "traffic"} <= set(k) for k in full["kernels"])


def test_bench_plain_run_times_its_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """The driver's call (no --full): the contract keys and nothing that needs runs of its own, the steps it was asked for,
    no side file; --dump-outputs writes the codes and every encoder weight gradient of the last timed step, float32, within
    64 MB (arrays over bench.DUMP_MAX_ENTRIES entries as a fixed sample of that many)."""
    import numpy as np
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert {"metric", "unit", "higher_is_better", "dtype"} <= set(d)
    assert not {"roofline", "kernels", "cpu_baseline", "workloads", "train_steps", "steady_state", "details"} & set(d)
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert {"codes.npy", "grad_W_emb.npy", "grad_W_self1.npy", "grad_W_f2.npy", "grad_b_emb.npy"} <= set(files)
    assert "grad_W_relation.npy" not in files
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert files["codes.npy"].shape == (1 << 21,) and files["grad_W_self1.npy"].shape == (500, 500)
    assert np.abs(files["grad_W_self1.npy"]).max() > 0
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
