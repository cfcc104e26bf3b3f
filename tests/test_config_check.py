"""What rgcn_create refuses before it touches the device (csrc/config_check.h: pure host arithmetic on rgcn_config), pinned
without a GPU.  tests/sanitize/config_check_driver.cpp prints check_config()'s answer -- status|message -- for every named
configuration, built with g++ under AddressSanitizer and UndefinedBehaviorSanitizer; the expected lines below are literals,
copied by hand from the refusals as rgcn_create and block_geometry spelled them before the check had a module of its own.

Unless a name says otherwise a configuration is the parity tests' small shape (V 150, R 9, d 20, L 2, 4 blocks or 2 bases,
800 edges, keep probability 0.8, one GPU, embedding input) with one thing changed; `both_*` break two rules at once and pin
which one answers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK = "0|"
INVALID, UNSUPPORTED = "1|", "5|"
POSITIVE = INVALID + "EntityCount, RelationCount, dimension, NumberOfLayers and NumberOfBasisFunctions must be positive"
NO_LAYERS = INVALID + "RGCN_KIND_EMBEDDING has no layers: num_layers must be 0 and num_bases 1"
KEEP = INVALID + "DropoutKeepProbability must be in (0,1]"
RANK = INVALID + "need 0 <= rank < world"
EDGES = INVALID + "max_edges out of range"
SORT_KEYS = UNSUPPORTED + "EntityCount and 2 x RelationCount must be below 2^24 (sort key range of this build)"
TOO_LARGE = UNSUPPORTED + "problem too large for this build"
BLOCK_SIZE = UNSUPPORTED + "block size d/nb must be one of 1,2,3,4,5,8"
BLOCKS = UNSUPPORTED + "NumberOfBasisFunctions (block count) > 512"
INDIVISIBLE = INVALID + ("InternalEncoderDimension must be divisible by NumberOfBasisFunctions "
                         "(the reference silently mis-groups otherwise: gcn_basis_concat.py:15,42)")
TDIAG_SHARDED = UNSUPPORTED + ("RGCN_KIND_BASIS_TDIAG on a sharded context (the products P, dP and the coefficient "
                               "table have no exchange points)")
TDIAG_2_31 = UNSUPPORTED + "RGCN_KIND_BASIS_TDIAG: 2 x EntityCount x NumberOfBasisFunctions x dimension must be below 2^31"
PDIAG_2_31 = UNSUPPORTED + "RGCN_KIND_BASIS_PDIAG: 2 x EntityCount x NumberOfBasisFunctions x dimension must be below 2^31"
ONEHOT_BLOCK = UNSUPPORTED + ("RGCN_INPUT_ONEHOT with the block kind: the reference's one-hot branch of ConcatGcn "
                              "cannot execute (gcn_basis_concat.py:18-19,42-46)")
ONEHOT_SHARDED = UNSUPPORTED + "RGCN_INPUT_ONEHOT on a sharded context (the [V,B,d] tables are not sharded)"

EXPECTED = {
    "ok_block": OK, "ok_basis": OK, "ok_basis_onehot": OK, "ok_block_highway": OK, "ok_basis_highway": OK, "ok_tdiag": OK,
    "ok_pdiag": OK, "ok_embedding": OK, "ok_block_sharded": OK, "ok_basis_local_norm": OK,
    "abi": INVALID + "abi_version mismatch",
    "zero_entities": POSITIVE, "zero_relations": POSITIVE, "zero_dim": POSITIVE, "zero_layers": POSITIVE, "zero_bases": POSITIVE,
    "embedding_with_a_layer": NO_LAYERS, "embedding_two_bases": NO_LAYERS,
    "keep_0": KEEP, "keep_1": OK, "keep_above_1": KEEP, "keep_negative": KEEP,
    "kind_5": INVALID + "unknown kind", "kind_negative": INVALID + "unknown kind",
    "norm_negative": INVALID + "unknown norm_mode", "norm_4": INVALID + "unknown norm_mode",
    "world_0": RANK, "rank_negative": RANK, "rank_is_world": RANK, "rank_0_of_2": OK,
    "edges_negative": EDGES, "edges_500m": OK, "edges_500m_and_1": EDGES,
    "input_mode_2": INVALID + "unknown input_mode (0: embedding input, 1: RGCN_INPUT_ONEHOT)",
    "embedding_sharded": UNSUPPORTED + "RGCN_KIND_EMBEDDING on a sharded context (nothing to shard by relation)",
    "embedding_onehot": UNSUPPORTED + "RGCN_KIND_EMBEDDING with RGCN_INPUT_ONEHOT (there is no first layer)",
    "embedding_highway": UNSUPPORTED + "RGCN_KIND_EMBEDDING with RGCN_SKIP_HIGHWAY (there is no layer to skip)",
    "tdiag_sharded": TDIAG_SHARDED,
    "tdiag_onehot": UNSUPPORTED + ("RGCN_KIND_BASIS_TDIAG with RGCN_INPUT_ONEHOT (the reference's one-hot branch of "
                                   "BasisGcnTimesDiag exists, gcn_basis_times_diag.py:21,70,76: not built)"),
    "tdiag_highway": UNSUPPORTED + "RGCN_KIND_BASIS_TDIAG with RGCN_SKIP_HIGHWAY (not built)",
    "tdiag_64_bases": OK,
    "tdiag_65_bases": UNSUPPORTED + "NumberOfBasisFunctions > 64 (basis_tdiag)",
    "tdiag_below_2_31": OK, "tdiag_at_2_31": TDIAG_2_31,
    "pdiag_sharded": UNSUPPORTED + ("RGCN_KIND_BASIS_PDIAG on a sharded context (the mixing table, the diagonal aggregate "
                                    "and the diagonal tables' gradient have no exchange points)"),
    "pdiag_onehot": UNSUPPORTED + ("RGCN_KIND_BASIS_PDIAG with RGCN_INPUT_ONEHOT (the one-hot first layer of "
                                   "BasisGcnWithDiag is not built)"),
    "pdiag_highway": UNSUPPORTED + "RGCN_KIND_BASIS_PDIAG with RGCN_SKIP_HIGHWAY (not built)",
    "pdiag_64_bases": OK,
    "pdiag_65_bases": UNSUPPORTED + "NumberOfBasisFunctions > 64 (basis_pdiag)",
    "pdiag_below_2_31": OK, "pdiag_at_2_31": PDIAG_2_31,
    "onehot_block": ONEHOT_BLOCK, "onehot_sharded": ONEHOT_SHARDED,
    "onehot_below_2_31": OK,
    "onehot_at_2_31": UNSUPPORTED + "RGCN_INPUT_ONEHOT: EntityCount x NumberOfBasisFunctions x dimension must be below 2^31",
    "highway_sharded": UNSUPPORTED + "RGCN_SKIP_HIGHWAY on a sharded context (the highway passes have no exchange points)",
    "highway_onehot": UNSUPPORTED + ("RGCN_SKIP_HIGHWAY with RGCN_INPUT_ONEHOT (in the reference the one-hot first layer "
                                     "gets no highway layer while the layers above it do: not built)"),
    "entities_2_24_less_1": OK, "entities_2_24": SORT_KEYS, "relations_2_23_less_1": OK, "relations_2_23": SORT_KEYS,
    "rows_times_dim_2_31": OK, "rows_times_dim_above_2_31": TOO_LARGE,
    "messages_times_dim_below_2_40": OK, "messages_times_dim_above_2_40": TOO_LARGE,
    "block_3_of_20": INDIVISIBLE,
    "blocks_512": OK, "blocks_513": BLOCKS,
    "block_size_1": OK, "block_size_2": OK, "block_size_3": OK, "block_size_4": OK, "block_size_5": OK,
    "block_size_6": BLOCK_SIZE, "block_size_7": BLOCK_SIZE, "block_size_8": OK, "block_size_9": BLOCK_SIZE,
    "basis_64_bases": OK,
    "basis_65_bases": UNSUPPORTED + "NumberOfBasisFunctions > 64 (basis)",
    "basis_onehot_65_bases": UNSUPPORTED + "NumberOfBasisFunctions > 64 (basis)",
    # two rules at once: the one rgcn_create came to first
    "both_abi_and_zero_entities": INVALID + "abi_version mismatch",
    "both_embedding_layers_and_highway": NO_LAYERS,
    "both_keep_0_and_entities_2_24": KEEP,
    "both_unknown_kind_and_norm": INVALID + "unknown kind",
    "both_tdiag_sharded_and_onehot": TDIAG_SHARDED,
    "both_tdiag_65_bases_and_2_31": UNSUPPORTED + "NumberOfBasisFunctions > 64 (basis_tdiag)",
    "both_pdiag_highway_and_65_bases": UNSUPPORTED + "RGCN_KIND_BASIS_PDIAG with RGCN_SKIP_HIGHWAY (not built)",
    "both_onehot_block_and_highway": ONEHOT_BLOCK,
    "all_highway_onehot_sharded": ONEHOT_SHARDED,
    "both_blocks_513_and_indivisible": INDIVISIBLE,
    "both_blocks_513_and_block_size_6": BLOCKS,
}


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("config_check") / "config_check_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "config_check_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "config_check_driver: ok"
    got = dict(line.split(": ", 1) for line in lines[:-1])
    assert len(got) == len(lines) - 1, "a case name printed twice"
    return got


def test_config_check_table_under_asan_and_ubsan(verdicts):
    wrong = {k: (verdicts.get(k), v) for k, v in EXPECTED.items() if verdicts.get(k) != v}
    assert not wrong, "\n".join("%s:\n  got      %s\n  expected %s" % (k, g, e) for k, (g, e) in wrong.items())
    assert set(verdicts) == set(EXPECTED), sorted(set(verdicts) ^ set(EXPECTED))


def test_the_add_diagonal_kind_takes_64_bases_and_refuses_65(verdicts):
    """what csrc/basis_pdiag.hip's `const int b = threadIdx.x;      // (B <= 64)` and tests/pdiag_grid.py rest on"""
    assert verdicts["pdiag_64_bases"] == "0|"
    assert verdicts["pdiag_65_bases"] == "5|NumberOfBasisFunctions > 64 (basis_pdiag)"


def test_every_refusal_and_every_kind_is_in_the_table():
    """rgcn_create and block_geometry held 33 distinct refusal texts before the first HIP call: each is expected at least once"""
    assert len({v for v in EXPECTED.values() if v != OK}) == 33
    assert all(EXPECTED[k] == OK for k in EXPECTED if k.startswith("ok_"))
    assert sum(k.startswith(("both_", "all_")) for k in EXPECTED) >= 4
