"""The launch-form table of the dense contractions (tests/gemm_launch_grid.py) names every cell the GPU grid promises, its
float64 reference is the contraction it says it is, and its mirrors of the split arithmetic follow csrc/gemm_plan.h and the
kernels.  No GPU: an edit of the table that drops a cell fails here, naming the cell."""
import os

import numpy as np
import pytest

import gemm_launch_grid as gl
import test_gemm_plan

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
MODES = (0, 3, 6, 9)


def _plans(c):
    return {mode: gl.plan_mirror(c, mode) for mode in MODES}


# ------------------------------------------------------------------ the reference
def test_reference_is_the_grouped_strided_contraction():
    """build_operands lays the logical operands out as the call describes them, and reference() is einsum on what the
    strided buffers hold inside the extents -- on all three storage forms, with padding, gaps and both kinds of extent."""
    for form in gl.FORMS:
        for kw in (dict(limit=(3, 7, 0), limit_stride=2), dict(limit=(5, 0, 11), limit_on_k=True)):
            c = gl.case("x", "x", form, 7, 5, 11, groups=3, pad_a=2, pad_b=3, pad_c=1, gap_a=5, gap_b=2, gap_c=3, **kw)
            A, B = gl.logical_operands(c, 7)
            a, b, cbuf = gl.build_operands(c, A, B)
            g = gl.geometry(c)
            assert a.size == 2 * g["strideA"] + g["rows_a"] * g["lda"] and cbuf.size == 2 * g["strideC"] + 7 * g["ldc"]
            assert (cbuf.view(np.uint32) == gl.CANARY.view(np.uint32)).all()
            seen_a, seen_b = np.zeros(a.shape, bool), np.zeros(b.shape, bool)
            for grp, ((mlim, klim), (ref, mag)) in enumerate(zip(gl.extents(c), gl.reference(c, A, B))):
                av = np.lib.stride_tricks.as_strided(a[grp * g["strideA"]:], (g["rows_a"], g["cols_a"]), (4 * g["lda"], 4))
                bv = np.lib.stride_tricks.as_strided(b[grp * g["strideB"]:], (g["rows_b"], g["cols_b"]), (4 * g["ldb"], 4))
                opa = (av if g["a_kc"] else av.T).astype(np.float64)      # [M, K]
                opb = (bv.T if g["b_kc"] else bv).astype(np.float64)      # [K, N]
                want = np.einsum("mk,kn->mn", opa[:mlim, :klim], opb[:klim])
                assert ref.shape == (mlim, 5) and np.allclose(ref, want, rtol=1e-13, atol=0)
                assert np.allclose(mag, np.einsum("mk,kn->mn", np.abs(opa[:mlim, :klim]), np.abs(opb[:klim])), rtol=1e-13)
                # what lies beyond an extent is the sentinel, what lies inside is not
                assert (opa[mlim:] == gl.SENTINEL).all() and (opa[:, klim:] == gl.SENTINEL).all() and (opb[klim:] == gl.SENTINEL).all()
                assert (np.abs(opa[:mlim, :klim]) < 1e6).all() and (np.abs(opb[:klim]) < 1e6).all()
                ia = (grp * g["strideA"] + np.arange(g["rows_a"])[:, None] * g["lda"] + np.arange(g["cols_a"])[None, :]).ravel()
                ib = (grp * g["strideB"] + np.arange(g["rows_b"])[:, None] * g["ldb"] + np.arange(g["cols_b"])[None, :]).ravel()
                seen_a[ia] = True
                seen_b[ib] = True
            # padding columns and the gaps between groups
            assert (a[~seen_a] == gl.SENTINEL).all() and (~seen_a).sum() > 0
            assert (b[~seen_b] == gl.SENTINEL).all() and (~seen_b).sum() > 0
            views, gaps = gl.product_views(c, cbuf)
            assert len(views) == 3 and views[1].shape == (7, g["ldc"]) and gaps.sum() == 2 * 3
            lim = gl.limit_array(c)
            assert lim.size == 2 * c["limit_stride"] + 1 and tuple(lim[::c["limit_stride"]]) == c["limit"]


# ------------------------------------------------------------------ the mirrors
def _pinned(name):
    return dict(f.split("=") for f in test_gemm_plan.EXPECTED[name].split()[1:])


def test_split_mirror_reproduces_the_pinned_plan_lines():
    p = _pinned("tn_split8")
    assert gl.plan_split(14541, 8) == (int(p["splits"]), int(p["kps"])) == (8, 1824)
    p = _pinned("n5_b_off4_split4_k16")
    assert gl.plan_split(16, 4) == (int(p["splits"]), int(p["kps"])) == (1, 16)
    p = _pinned("limit_on_k_split8")
    assert gl.plan_split(14541, 8) == (int(p["splits"]), int(p["kps"]))
    assert gl.plan_split(500, 1) == (1, 512) and gl.plan_split(5, 3) == (1, 16) and gl.plan_split(33, 3) == (3, 16)
    assert gl.plain_slices(33, 3) == [(0, 16), (16, 32), (32, 33)]
    # the device divides the actual depth over the plan's slice count
    assert gl.device_slices(120, 3, 77) == [(0, 32), (32, 64), (64, 77)] and gl.slices_coincide(120, 3, 77)
    assert gl.device_slices(120, 8, 20) == [(0, 16), (16, 20)] + [(16 * z, 16 * z) for z in range(2, 8)]
    assert gl.slices_coincide(120, 8, 20)
    assert gl.device_slices(100, 5, 68) == [(0, 32), (32, 64), (64, 68), (96, 96)] and not gl.slices_coincide(100, 5, 68)
    assert gl.device_slices(120, 3, 0) == [(0, 0), (16, 16), (32, 32)]


def test_plan_mirror_reproduces_pinned_lines_of_the_decision_table():
    """the alignment and table cells of tests/test_gemm_plan.py, restated as cases of this table"""
    def line(c, mode=6):
        p = gl.plan_mirror(c, mode)
        a_kc, b_kc = gl.FORMS[c["form"]]
        return "%s<%d,%d> terms=%d vec=%d table=%d pro=0 swz=%d splits=%d kps=%d slabs=%d ldc=%d vecC=%d tiles=%dx%d grid=%d" % (
            p["kernel"], a_kc, b_kc, p["terms"], p["vec"], p["table"], p["swizzle"], p["splits"], p["k_per_split"], p["slabs"],
            p["ldc"], p["vecC"], p["tiles_m"], p["tiles_n"], p["grid_x"])
    E = test_gemm_plan.EXPECTED
    assert line(gl.case("x", "x", "TN", 500, 500, 14541, split_k=8)) == E["tn_split8"]
    assert line(gl.case("x", "x", "TN", 500, 500, 14541, split_k=8), 0) == E["mode0_tn_split8"]
    assert line(gl.case("x", "x", "NN", 256, 128, 500, off_a=1, table="presplit")) == E["a_off4"]
    assert line(gl.case("x", "x", "NN", 256, 128, 500, pad_a=2, table="presplit")) == E["lda502"]
    assert line(gl.case("x", "x", "NN", 256, 5, 500, off_b=1, table="presplit")) == E["n5_b_off4"]
    assert line(gl.case("x", "x", "NN", 256, 5, 16, off_b=1, split_k=4, table="presplit")) == E["n5_b_off4_split4_k16"]
    assert line(gl.case("x", "x", "NT", 14541, 500, 500, table="w8")) == E["nt_knob3"]
    assert line(gl.case("x", "x", "NT", 14541, 500, 500, table="presplit")) == E["nt_knob0"]
    assert line(gl.case("x", "x", "NN", 14541, 500, 500, table="w8"), 3) == E["mode3_knob3"]
    assert line(gl.case("x", "x", "NN", 1100, 500, 500, groups=2, limit=(1, 2), table="w8")) == E["groups_row_limit"]
    assert line(gl.case("x", "x", "NN", 1100, 500, 500, groups=2, limit=(1, 2), gap_a=1, table="w8")) == E["groups_row_limit_strideA_odd"]
    assert line(gl.case("x", "x", "NN", 1100, 500, 500, groups=2, limit=(1, 2), gap_c=1, table="w8")) == E["groups_row_limit_strideC_odd"]
    assert line(gl.case("x", "x", "NN", 256, 128, 500, limit=(7,), limit_on_k=True, table="w8")) == E["limit_on_k_knob3"]
    assert "refused: " + gl.plan_mirror(gl.case("x", "x", "TN", 500, 500, 14541, split_k=8, limit=(3,)), 6) == E["row_limit_split8"]


@pytest.mark.parametrize("source,text", [
    ("gemm_plan.h", "const int want = q.split_k < 1 ? 1 : q.split_k;"),
    ("gemm_plan.h", "int kps = (q.K + want - 1) / want;"),
    ("gemm_plan.h", "kps = ((kps + kGemmBK - 1) / kGemmBK) * kGemmBK;"),
    ("gemm_plan.h", "p.splits = q.K > 0 ? (q.K + kps - 1) / kps : 1;"),
    ("gemm_plan.h", "constexpr int kGemmBK = 16, kGemmBM = 128, kGemmBN = 128, kGemmWideBN = 256;"),
    ("gemm_f32.hip", "const int per = (Klim + g.splits - 1) / g.splits;"),
    ("gemm_f32.hip", "kps = max(BK, ((per + BK - 1) / BK) * BK);"),
    ("gemm_bf16x3.hip", "const int per = (Klim + g.splits - 1) / g.splits;"),
    ("gemm_bf16x3.hip", "kps = max(BK, ((per + BK - 1) / BK) * BK);"),
    ("gemm_f32.hip", "if (N % 4 == 0 && q.ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(q.C) & 15u) == 0 && gsc % 4 == 0)"),
    ("gemm_f32.hip", "for (; s + 8 <= splits; s += 8) {"),
    ("rgcn_api.hip", "size_t slab = 64 * (size_t)c->d * c->d;"),
])
def test_host_mirrors_follow_the_sources(source, text):
    with open(os.path.join(CSRC, source)) as f:
        assert text in f.read(), "%s no longer holds `%s`: update tests/gemm_launch_grid.py's mirror" % (source, text)


# ------------------------------------------------------------------ every cell has a case
def test_cases_are_small_and_fit_the_engine():
    assert gl.SLAB_FLOATS == 64 * gl.ENGINE[2] ** 2
    for name, c in gl.CASES.items():
        assert c["M"] in gl.SHAPES and c["N"] in gl.SHAPES and 1 <= c["K"] <= 300, name
        splits = gl.plan_split(c["K"], c["split_k"])[0]
        assert splits == 1 or c["groups"] * splits * c["M"] * c["N"] <= gl.SLAB_FLOATS, name
        assert all(0 <= c[k] <= 3 for k in ("off_a", "off_b", "off_c")), name
        for mlim, klim in gl.extents(c):
            assert 0 <= mlim <= c["M"] and 0 <= klim <= c["K"], name
        assert not isinstance(gl.plan_mirror(c, 6), str), name      # no case of the grid is a refused call
        # 16-byte loads of a k-contiguous operand take an extent on K in multiples of 4 only (GemmBatch::limit_on_k)
        if c["limit_on_k"] and c["form"] != "TN":
            for mode, p in _plans(c).items():
                assert not p["vec"] or all(k % 4 == 0 for _, k in gl.extents(c)), (name, mode)
    for c in gl.REFUSED_CASES:
        assert all(isinstance(p, str) for p in _plans(c).values()), c["name"]


def test_split_cell_names_every_count_tail_and_reduce_kernel():
    cases = gl.cases_of("split")
    for form in gl.FORMS:
        mine = [c for c in cases if c["form"] == form]
        for s in gl.SPLIT_COUNTS:
            got = {gl.plan_split(c["K"], c["split_k"])[0] for c in mine if c["split_k"] == s}
            assert s in got, "%s: no case runs %d slices" % (form, s)
            assert any(x < s for x in got), "%s: no case asks for %d slices and gets fewer" % (form, s)
            last = [gl.plain_slices(c["K"], s)[-1] for c in mine if c["split_k"] == s and gl.plan_split(c["K"], s)[0] == s]
            assert any((ke - ks) % gl.BK for ks, ke in last), "%s split %d: no partial last k-tile" % (form, s)
            assert any(ke - ks == gl.plan_split(c["K"], s)[1] for c in mine if c["split_k"] == s
                       for ks, ke in [gl.plain_slices(c["K"], s)[-1]]), "%s split %d: no exactly full last slice" % (form, s)
            assert {gl.reduce_width(c) for c in mine if c["split_k"] == s} >= {1, 4}, "%s split %d: a reduce kernel is missing" % (form, s)
        assert any(c["pad_c"] > 0 and gl.reduce_width(c) == 4 for c in mine), form
        assert any(c["pad_c"] > 0 and gl.reduce_width(c) == 1 for c in mine), form
        assert any(c["N"] == 5 and gl.reduce_width(c) == 1 for c in mine), form
        assert any(gl.plain_slices(c["K"], c["split_k"])[0][1] > gl.BK for c in mine), "%s: no slice of several k-tiles" % form
    # eight slabs at a time, then the tail: 8 -> one round, 9 -> a round and one, 17 -> two rounds and one
    assert {gl.plan_split(c["K"], c["split_k"])[0] for c in cases} >= {2, 3, 8, 9, 17}


def test_group_cell_names_two_and_three_groups_on_every_kernel():
    cases = gl.cases_of("groups")
    reached = {(c["groups"], p["kernel"]) for c in cases for p in _plans(c).values()}
    for n in (2, 3):
        for kernel in ("f32", "staged", "presplit", "w8"):
            assert (n, kernel) in reached, "no case runs %d groups on the %s kernel" % (n, kernel)
    for c in cases:
        assert c["gap_a"] > 0 and c["gap_b"] > 0 and c["gap_c"] > 0, c["name"]      # strides larger than the operand
    assert any(gl.reduce_width(c) == 4 and c["groups"] > 1 for c in cases)
    assert any(gl.reduce_width(c) == 1 and c["groups"] > 1 for c in cases)
    assert any(gl.plan_mirror(c, 6)["vec"] == 0 for c in cases) and any(gl.plan_mirror(c, 6)["vecC"] == 0 for c in cases)
    assert {c["form"] for c in cases} == set(gl.FORMS)


def test_row_extent_cell_names_every_extent_on_every_kernel():
    cases = gl.cases_of("row_extent")
    reached = set()
    for c in cases:
        M = c["M"]
        assert {0, 1, M - 3, M} <= set(c["limit"]), c["name"]
        assert any(gl.ceil_div(n, gl.BM) < gl.ceil_div(M, gl.BM) and n > 1 for n in c["limit"]), c["name"]   # a whole panel left out
        assert c["limit_stride"] > 1, c["name"]
        for p in _plans(c).values():
            assert p["swizzle"] == 2, c["name"]
            reached.add((p["kernel"], c["form"]))
    assert 129 in {c["M"] for c in cases}
    for kernel, forms in (("f32", gl.FORMS), ("staged", gl.FORMS), ("presplit", ("NN", "NT")), ("w8", ("NN", "NT"))):
        for form in forms:
            assert (kernel, form) in reached, "no row-extent case on %s %s" % (kernel, form)
    assert gl.REFUSED_CASES and all(c["split_k"] > 1 and c["limit"] is not None and not c["limit_on_k"] for c in gl.REFUSED_CASES)


def test_depth_extent_cell_names_split_and_unsplit_zero_and_both_slice_relations():
    cases = gl.cases_of("depth_extent")
    for form in gl.FORMS:
        mine = [c for c in cases if c["form"] == form]
        assert any(gl.plan_split(c["K"], c["split_k"])[0] > 1 for c in mine), form
        assert any(gl.plan_split(c["K"], c["split_k"])[0] == 1 for c in mine), form
    for c in cases:
        assert c["groups"] == 2 and c["limit"][0] != c["limit"][1] and c["limit_on_k"], c["name"]
    assert sum(0 in c["limit"] for c in cases) >= len(cases) - 2
    assert any(k % 4 for c in cases for k in c["limit"])
    rel = {gl.slices_coincide(c["K"], c["split_k"], k) for c in cases for k in c["limit"] if k > 0}
    assert rel == {True, False}
    kernels = {p["kernel"] for c in cases for p in _plans(c).values()}
    assert kernels == {"f32", "staged", "presplit"}      # never the eight-wavefront kernel
    assert any(c["table"] == "w8" for c in cases)


def test_layout_cells_name_padding_and_every_misaligned_base():
    for form in gl.FORMS:
        ld4 = [c for c in gl.cases_of("ld_plus_4") if c["form"] == form]
        assert ld4 and all(c["pad_a"] == c["pad_b"] == c["pad_c"] == 4 for c in ld4)
        for c in ld4:
            for mode, p in _plans(c).items():
                assert p["vec"] == 1 and p["vecC"] == 1, (c["name"], mode)
        assert any(gl.plan_split(c["K"], c["split_k"])[0] > 1 for c in ld4), form
        ld1 = [c for c in gl.cases_of("ld_plus_1") if c["form"] == form]
        assert ld1 and all(c["pad_a"] == 1 and gl.geometry(c)["cols_a"] % 4 for c in ld1)
        assert all(p["vec"] == 0 and p["table"] == 0 for c in ld1 for p in _plans(c).values())
        for cell, key in (("offset_a", "off_a"), ("offset_b", "off_b"), ("offset_c", "off_c")):
            mine = [c for c in gl.cases_of(cell) if c["form"] == form]
            assert mine and all(c[key] % 4 for c in mine), (cell, form)
    kernels = {p["kernel"] for c in gl.cases_of("ld_plus_4") for p in _plans(c).values()}
    assert kernels == {"f32", "staged", "presplit", "w8"}
    # a misaligned A switches the table off; a misaligned B behind its table does not matter (NN), elsewhere it does
    for c in gl.cases_of("offset_a"):
        assert all(p["vec"] == 0 and p["table"] == 0 for p in _plans(c).values()), c["name"]
    offb = {c["form"]: gl.plan_mirror(c, 6) for c in gl.cases_of("offset_b")}
    assert offb["NN"]["vec"] == 1 and offb["NN"]["table"] == 1 and offb["NT"]["vec"] == 0 and offb["NT"]["table"] == 0
    assert offb["TN"]["vec"] == 0
    for c in gl.cases_of("offset_c"):
        for p in _plans(c).values():
            assert p["vecC"] == (1 if p["slabs"] else 0), c["name"]      # the slabs are aligned, the reduce stores dwords
        assert gl.reduce_width(c) in (0, 1)
    assert any(gl.reduce_width(c) == 1 for c in gl.cases_of("offset_c"))
