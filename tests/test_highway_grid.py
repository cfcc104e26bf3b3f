"""The highway case table (tests/highway_grid.py) covers every launch shape of csrc/highway.hip's kernels, every loop of
theirs beyond its first trip and every boundary of their dispatch; the mirrors follow the kernel source; and a plain
float32 numpy evaluation of the float64 restatement passes, on every case's inputs, the very checks
tests/test_gpu_highway_grid.py applies -- the condition its bounds rest on.  No GPU: a later edit of the table that
drops a cell fails here, naming the cell."""
import os
import re

import numpy as np
import pytest

import highway_grid as hg
import highway_reference as hr
from helpers import assert_close
from kernel_grid import BLOCK_SIZES, row_slots
from tdiag_grid import auto_split_k

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
GRID = hg.HIGHWAY_GRID_LIST
FWD_ATOL = 1e-4              # tests/test_gpu_highway.py's, which tests/test_gpu_highway_grid.py imports


def _with(pred):
    return {hg.vec_of(c["d"]) for c in GRID if pred(c)}


def _both(pred, what):
    have = _with(pred)
    assert have == set(hg.VECS), "VEC with a case of %s: %s" % (what, sorted(have))


# ----------------------------------------------------------------------------- cell coverage
def test_one_column_lane_and_256_column_lanes_are_in_the_table():
    assert hg.cell_of(hg.HIGHWAY_GRID["hw_d4"])[:2] == (4, 1) and hg.row_lanes(4) == 256
    _both(lambda c: hg.column_lanes(c["d"]) == 256 and hg.row_lanes(c["d"]) == 1, "CL = 256")
    lanes = {hg.column_lanes(c["d"]) for c in GRID}
    assert {1, 2, 8, 128, 256} <= lanes
    # what tests/test_gpu_highway.py reaches: CL 2 (d = 8), CL 16 (d = 10), CL 128 (d = 500), one chunk, one row trip
    assert [hg.column_lanes(d) for d in (8, 10, 500)] == [2, 16, 128]
    assert hg.column_chunks(500) == 1 and hg.row_trips(257, 500) == 1 and hg.fwd_trips(257, 500) == 1


def test_every_dispatch_boundary_is_in_the_table():
    widths = {c["d"] for c in GRID if c["V"] == 300}
    missing = [(vec, d) for vec in hg.VECS for d in hg.BOUNDARY_WIDTHS[vec] if d not in widths]
    assert not missing, "dispatch boundaries (VEC, d) without a case: %s" % missing
    assert [hg.nvec_of(d) for d in hg.BOUNDARY_WIDTHS[4]] == [128, 129, 256, 257]
    assert [hg.nvec_of(d) for d in hg.BOUNDARY_WIDTHS[1]] == [127, 129, 255, 257]       # (128 and 256 are VEC 4 widths)
    for vec in hg.VECS:
        assert all(hg.vec_of(d) == vec for d in hg.BOUNDARY_WIDTHS[vec])
        assert [(hg.column_lanes(d), hg.column_chunks(d)) for d in hg.BOUNDARY_WIDTHS[vec]] == [(128, 1), (256, 1), (256, 1), (256, 2)]
    assert hg.vec_of(128) == 4 and hg.vec_of(256) == 4


def test_an_exact_power_of_two_and_a_ragged_width_are_in_the_table_for_both_vector_widths():
    _both(lambda c: hg.column_lanes(c["d"]) == hg.nvec_of(c["d"]) > 1, "no dead lane (nvec a power of two above 1)")
    _both(lambda c: hg.column_lanes(c["d"]) > hg.nvec_of(c["d"]), "dead lanes")


def test_every_loop_has_a_case_at_one_trip_and_a_case_at_two():
    for what, count in (("column chunks", lambda c: hg.column_chunks(c["d"])),
                        ("row trips", lambda c: hg.row_trips(c["V"], c["d"])),
                        ("forward trips", lambda c: hg.fwd_trips(c["V"], c["d"]))):
        _both(lambda c: count(c) == 1, "%s = 1" % what)
        _both(lambda c: count(c) >= 2, "%s >= 2" % what)
    # the second column chunk has one live lane
    _both(lambda c: hg.column_chunks(c["d"]) == 2 and hg.nvec_of(c["d"]) - hg.column_lanes(c["d"]) == 1, "nvec = 257")
    for vec in hg.VECS:
        r, f = hg.HIGHWAY_GRID[hg.ROW_TRIPS[vec]], hg.HIGHWAY_GRID[hg.FWD_TRIPS[vec]]
        assert hg.vec_of(r["d"]) == hg.vec_of(f["d"]) == vec
        # CL = 256 and V > 1024: the grid is capped, the row loop takes a second trip, 1024 partial rows are summed
        assert hg.column_lanes(r["d"]) == 256 and hg.row_grid(r["V"], r["d"]) == hg.HW_MAX_BLOCKS and hg.row_trips(r["V"], r["d"]) == 2
        assert hg.fwd_trips(f["V"], f["d"]) == 2 and hg.fwd_trips(f["V"] - 100, f["d"]) == 1 and f["L"] == 1 and f["nb"] == 1
    assert hg.row_trips(1024, 1028) == 1 and hg.row_trips(1025, 1028) == 2


def test_the_forward_trip_cases_split_the_basis_weight_gradient_into_more_than_16_slabs():
    """gemm_basis_dw (rgcn_schedule.hip: `auto_split_k(2 * Bd, d, V)`, two groups) at one basis function, few tiles and many
    rows asks for 35 slabs a group, 70 d^2 floats: more than the 64 d^2 a context used to allocate (rgcn_create once sized
    them for 16 a group), so the backward pass of these two cases was refused before rgcn_create followed auto_split_k"""
    for vec in hg.VECS:
        c = hg.HIGHWAY_GRID[hg.FWD_TRIPS[vec]]
        split = auto_split_k(2 * c["nb"] * c["d"], c["d"], c["V"])
        assert split == 35 and 2 * split * c["nb"] > 64
    assert all(2 * auto_split_k(2 * c["nb"] * c["d"], c["d"], c["V"]) * c["nb"] <= 64 for c in GRID if c["V"] <= 1100 and c["kind"] == "basis")
    with open(os.path.join(CSRC, "rgcn_api.hip")) as f:
        assert "std::max(16, auto_split_k((int)zc, (int)d, (int)V)) * zc * d" in f.read()


def test_rows_that_do_not_fill_the_row_lanes_and_three_layers_at_width_are_in_the_table():
    ragged = [c["name"] for c in GRID if hg.row_lanes(c["d"]) > 1 and c["V"] % hg.row_lanes(c["d"]) != 0]
    assert "hw_d4" in ragged and "hw_d2" in ragged
    deep = [c for c in GRID if c["L"] == 3]
    assert deep and all(hg.column_lanes(c["d"]) == 256 for c in deep)


def test_the_block_case_has_a_compiled_block_size_at_256_column_lanes():
    blocks = [c for c in GRID if c["kind"] == "block"]
    assert len(blocks) == 1
    c = blocks[0]
    assert c["d"] % c["nb"] == 0 and c["d"] // c["nb"] in BLOCK_SIZES and hg.column_lanes(c["d"]) == 256
    assert all(c["nb"] in (1, 2) for c in GRID if c["kind"] == "basis")


def test_the_named_cases_are_what_their_names_say():
    for vec in hg.VECS:
        widest = max((c for c in GRID if hg.vec_of(c["d"]) == vec and c["V"] == 300), key=lambda c: c["d"])
        assert hg.HIGHWAY_GRID[hg.WIDEST[vec]] is widest and hg.column_chunks(widest["d"]) == 2
    assert hg.column_lanes(hg.HIGHWAY_GRID[hg.GEMM_MODE_0]["d"]) == 256
    assert len(hg.HIGHWAY_GRID) == len(GRID)


def test_mirrors_on_known_configurations():
    assert [hg.cell_of(hg.HIGHWAY_GRID[n]) for n in ("hw_d4", "hw_d20", "hw_d516", "hw_d1028", "hw_d2", "hw_d257",
                                                     "hw_rows_vec4", "hw_fwd_vec1")] == [
        (4, 1, 1, 1, 1), (4, 8, 1, 1, 1), (4, 256, 1, 1, 1), (4, 256, 2, 1, 1), (1, 2, 1, 1, 1), (1, 256, 2, 1, 1),
        (4, 256, 2, 2, 1), (1, 256, 2, 9, 2)]
    assert [hg.row_grid(300, d) for d in (4, 20, 512, 516, 2)] == [2, 10, 150, 300, 3]
    assert [hg.fwd_trips(V, d) for V, d in ((8160, 257), (8161, 257), (32263, 260), (32264, 260))] == [1, 2, 1, 2]


@pytest.mark.parametrize("name", sorted(hg.HIGHWAY_GRID))
def test_case_graph_has_its_hub_rows(name):
    c = hg.HIGHWAY_GRID[name]
    t = hg.case_inputs(c)["triples"]
    assert t.shape == (c["E"], 3) and t.dtype == np.int32 and (c["R"], c["E"]) == (237, 3000)
    assert tuple(row_slots(t, c["V"])[:3]) == hg.HUBS
    assert c["V"] == 300 or name in list(hg.ROW_TRIPS.values()) + list(hg.FWD_TRIPS.values())


# ----------------------------------------------------------------------------- the mirrors follow the source
@pytest.mark.parametrize("pattern,count", [
    (r"constexpr int kHwThreads = 256;", 1),
    (r"constexpr int kHwMaxBlocks = 1024;", 1),
    (r"while \(cl < nvec && cl < kHwThreads\) cl \*= 2;", 1),
    (r"const int RL = kHwThreads / CL;", 2),
    (r"const int CL = a\.CL, RL = kHwThreads / CL;", 1),
    (r"int64_t g = \(\(int64_t\)c->V \+ RL - 1\) / RL;\s+if \(g > kHwMaxBlocks\) g = kHwMaxBlocks;", 1),
    (r"for \(int c0 = 0; c0 < nvec; c0 \+= CL\) \{", 2),
    (r"r < (a\.)?V; r \+= \(int64_t\)gridDim\.x \* RL\) \{", 2),
    (r"int64_t grid = \(nvec \+ kHwThreads - 1\) / kHwThreads;\s+if \(grid > 8192\) grid = 8192;", 1),
    (r"__shared__ float red\[kHwThreads \* VEC\];", 2),
    (r"hw_column_lanes\(vec4 \? c->d / 4 : c->d\)", 2),
])
def test_host_mirrors_follow_the_kernel_source(pattern, count):
    """The mirrors in highway_grid.py are copies of these lines: when one changes, the table has to be re-derived."""
    with open(os.path.join(CSRC, "highway.hip")) as f:
        found = len(re.findall(pattern, f.read()))
    assert found == count, "highway.hip holds `%s` %d times, not %d: update tests/highway_grid.py's mirror" % (pattern, found, count)


def test_the_compiled_variants_are_both_vector_widths():
    with open(os.path.join(CSRC, "highway.hip")) as f:
        text = f.read()
    for k in ("k_highway_fwd", "k_highway_bwd", "k_highway_join"):
        assert set(re.findall(k + r"<(\d)>", text)) == {"4", "1"}, k


# ----------------------------------------------------------------------------- the float32 condition
@pytest.mark.parametrize("name", [c["name"] for c in GRID])
def test_float32_passes_the_gpu_checks(name):
    """what tests/test_gpu_highway_grid.py's check asks of the engine, asked of a plain float32 evaluation: H_l, N_l, T_l
    within FWD_ATOL of float64, every gradient within assert_close's defaults of the float64 reverse mode at the float32
    activations"""
    c = hg.case_inputs(hg.HIGHWAY_GRID[name])
    kind, V, L = c["kind"], c["V"], c["L"]
    kw = dict(mode="train", keep=c["keep"], masks=c["masks"])
    A64 = hr.forward(kind, c["params"], c["triples"], V, L, **kw)
    A32 = hr.forward_float32(kind, c["params"], c["triples"], V, L, **kw)
    for l in range(1, L + 1):
        errs = [float(np.abs(a32[l] - a64[l]).max()) for a32, a64 in zip(A32, A64)]
        print("%s layer %d: float32 vs float64 max abs H %.3e, N %.3e, T %.3e (max |H| %.3g)" % (
            (name, l) + tuple(errs) + (float(np.abs(A64[0][l]).max()),)))
        assert max(errs) <= FWD_ATOL, (name, l, errs)
    g32 = hr.backward(kind, c["params"], c["triples"], V, L, *A32, c["dcodes"], dtype=np.float32, **kw)
    g64 = hr.backward(kind, c["params"], c["triples"], V, L, *A32, c["dcodes"], **kw)
    for n in hr.weight_names(kind, L)[:-1]:
        assert g32[n].dtype == np.float32, n
        assert_close(g32[n], g64[n], name="%s %s" % (name, n))
