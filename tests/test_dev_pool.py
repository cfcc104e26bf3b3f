"""DevPool (csrc/dev_pool.h), the owner of the library's device allocations, against a fake HIP runtime -- host code only,
so it is pinned here without a GPU.  tests/sanitize/dev_pool_driver.cpp defines hipMalloc / hipFree / hipMemsetAsync over
malloc with a set of live blocks and a switch that fails the k-th allocation; it is built with g++ under AddressSanitizer
and UndefinedBehaviorSanitizer as a stand-alone program and prints one line per case.  The fake hipFree aborts on a pointer
that is not live, so a double free cannot pass, and LeakSanitizer sees whatever a pool forgets."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")

CASES = ["zero_elements", "zeroing", "release_once", "destructor", "move", "swap", "fail_nomem", "fail_other", "fail_memset"]

pytestmark = [
    pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available"),
    pytest.mark.skipif(not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime_api.h")),
                       reason="HIP runtime headers not found"),
]

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dev_pool") / "dev_pool_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-D__HIP_PLATFORM_AMD__",
           "-I" + ROCM_INCLUDE, "-x", "c++", os.path.join(ROOT, "tests", "sanitize", "dev_pool_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_dev_pool_cases_under_asan_and_ubsan(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=ENV, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-4000:]
    assert "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert lines[:-1] == [c + " ok" for c in CASES], run.stdout
    # every block the fake runtime handed out came back exactly once
    tally = dict(kv.split("=") for kv in lines[-1].split())
    assert int(tally["mallocs"]) > 0 and tally["mallocs"] == tally["frees"] and tally["live"] == "0", lines[-1]


@pytest.mark.parametrize("mode", ["double_free", "unknown_free"])
def test_fake_runtime_aborts_on_a_bad_free(driver, mode):
    """what makes "freed exactly once" checkable: the driver's hipFree refuses a pointer that is not live"""
    run = subprocess.run([driver, mode], capture_output=True, text=True, env=ENV, timeout=60)
    assert run.returncode != 0
    assert "is not a live block" in run.stderr, run.stderr[-2000:]
