"""The reciprocal pass's host-and-device decision text (csrc/negative_reciprocal.h) under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone driver (tests/sanitize/negative_reciprocal_driver.cpp) runs the kernel's loop
over buffers of exactly the batch's size and a guard, and its rows are the numpy mirror's
(tests/reciprocal_reference.py), row for row."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import reciprocal_reference as ref
import relation_negatives_reference as rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
# (n, rate, m): the thread counts 255 / 256 / 257 of the device test, tail rows only, one row, and a relation out of range
SHAPES = {"t255": (85, 2, 0), "t256": (64, 3, 0), "tail_only": (257, 0, 0), "one": (1, 3, 2), "t256_rel": (128, 1, 2)}
SEED = 2 ** 63 + 12345          # a seed above 2^63: the generator's arithmetic wraps, and must do so unsigned


def _case(name):
    V, R, batch, known = rel.small_fixture()
    n, rate, m = SHAPES[name]
    batch = batch[:n].copy()
    if name == "t255":
        batch[3, 1], batch[9, 1] = R, -1              # relations out of range: left as they are
    X0, Y0 = ref.sampler_rows("plain", batch, known, rate, m, V, R, SEED)
    return dict(n=n, rate=rate, m=m, R=R, batch=batch, X0=X0, Y0=Y0)


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("negative_reciprocal")
    exe = str(tmp / "negative_reciprocal_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "negative_reciprocal_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = []
    for name in sorted(SHAPES):
        c = _case(name)
        lines.append("case %s %d %d %d %d %d %d" % (name, c["n"], c["rate"], c["m"], c["R"], SEED, len(c["X0"])))
        lines += ["%d %d %d" % tuple(row) for row in c["batch"].tolist() + c["X0"].tolist()]
    path = tmp / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:] + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.splitlines()
    assert out[-1] == "negative_reciprocal_driver: ok"
    cases, cur = {}, None
    for line in out[:-1]:
        word = line.split()
        if word[0] == "case":
            cur = cases[word[1]] = {"total": int(word[3]), "rows": [], "choices": []}
        elif word[0] == "row":
            cur["rows"].append([int(word[1]), int(word[2]), int(word[3]), float(word[4])])
        elif word[0] == "choice":
            cur["choices"].append([int(word[1]), int(word[2]), int(word[3])])
    return cases


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_driver_equals_the_mirror(driver_output, name):
    c, got = _case(name), driver_output[name]
    n, rate, m, R = c["n"], c["rate"], c["m"], c["R"]
    X, Y = ref.transform(c["batch"], c["X0"], c["Y0"], rate, m, R, SEED)
    N = n * (rate + 2 + m)
    assert got["total"] == N == len(X)
    rows = np.array(got["rows"])
    assert len(rows) == N + GUARD
    assert np.array_equal(rows[:N, :3].astype(np.int64), X) and np.array_equal(rows[:N, 3], Y)
    assert (rows[N:] == -77).all()                                   # nothing behind the last row is written
    assert got["choices"] == [[i] + list(ref.choice(i, n, rate, m, R, SEED)) for i in range(-2, N + 2)]


def test_out_of_range_relations_pass_through(driver_output):
    c = _case("t255")
    rows = np.array(driver_output["t255"]["rows"])
    n, N = c["n"], c["n"] * (c["rate"] + 2)
    assert rows[N - n + 3, 1] == c["R"] and rows[N - n + 9, 1] == -1
    assert set(rows[n:N - n][3::n, 1].tolist()) == {c["R"]} and set(rows[n:N - n][9::n, 1].tolist()) == {-1}
