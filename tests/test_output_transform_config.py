"""What rgcn_create_ex refuses of the output transform (rgcn_config_ext::code_dim) before it touches the device
(csrc/config_check.h check_output_transform: pure host arithmetic, asked once check_config has accepted the configuration),
pinned without a GPU.  tests/sanitize/output_transform_config_driver.cpp prints the answer -- status|message -- for every
named configuration, built with g++ under AddressSanitizer and UndefinedBehaviorSanitizer as tests/test_config_check.py
builds its driver; the expected lines below are literals.

A configuration is test_config_check.py's small shape (V 150, R 9, d 20, L 2, 4 blocks or 2 bases, one GPU, embedding
input) with code_dim 8 and one thing changed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK = "0|"
INVALID, UNSUPPORTED = "1|", "5|"
NEGATIVE = INVALID + "code_dim must be 0 (no output transform) or the positive CodeDimension"
SHARDED = UNSUPPORTED + "code_dim > 0 on a sharded context (the gradient of W_out has no exchange point)"
EMBEDDING = UNSUPPORTED + ("code_dim > 0 with RGCN_KIND_EMBEDDING (the reference's embedding encoder has no output "
                           "transform, model_builder.py:27-41)")
ROWS_2_31 = UNSUPPORTED + "code_dim > 0: EntityCount x CodeDimension must be below 2^31"

EXPECTED = {
    "ok_block": OK, "ok_basis": OK, "ok_tdiag": OK, "ok_pdiag": OK, "ok_basis_onehot": OK, "ok_block_highway": OK,
    "ok_basis_highway": OK, "ok_wider": OK, "ok_equal_dimensions": OK,
    "none_block": OK, "none_block_sharded": OK, "none_embedding": OK,
    "negative": NEGATIVE, "negative_on_embedding": NEGATIVE,
    "sharded_block": SHARDED, "sharded_basis": SHARDED,
    "embedding_kind": EMBEDDING,
    "rows_times_code_dim_below_2_31": OK, "rows_times_code_dim_at_2_31": ROWS_2_31,
    "rows_times_code_dim_just_below_2_31": OK,
    # two rules at once: check_config's come first, then the layer's in the order of check_output_transform
    "both_unknown_kind_and_negative": INVALID + "unknown kind",
    "both_highway_sharded_and_code_dim": UNSUPPORTED + ("RGCN_SKIP_HIGHWAY on a sharded context (the highway passes have no "
                                                        "exchange points)"),
    "both_sharded_and_2_31": SHARDED,
}


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("output_transform_config") / "output_transform_config_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "output_transform_config_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "output_transform_config_driver: ok"
    got = dict(line.split(": ", 1) for line in lines[:-1])
    assert len(got) == len(lines) - 1, "a case name printed twice"
    return got


def test_output_transform_table_under_asan_and_ubsan(verdicts):
    wrong = {k: (verdicts.get(k), v) for k, v in EXPECTED.items() if verdicts.get(k) != v}
    assert not wrong, "\n".join("%s:\n  got      %s\n  expected %s" % (k, g, e) for k, (g, e) in wrong.items())
    assert set(verdicts) == set(EXPECTED), sorted(set(verdicts) ^ set(EXPECTED))


def test_every_refusal_is_in_the_table():
    """check_output_transform holds four refusal texts; each kind with layers is accepted once"""
    assert {NEGATIVE, SHARDED, EMBEDDING, ROWS_2_31} <= set(EXPECTED.values())
    assert all(EXPECTED[k] == OK for k in EXPECTED if k.startswith(("ok_", "none_")))
