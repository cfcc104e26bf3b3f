"""Every launch form of the dense contractions on its own (csrc/gemm_plan.h GemmCall / GemmBatch; gemm_f32.hip,
gemm_bf16x3.hip, gemm_bf16x3_w8.hip), through rgcn_debug_gemm_call: a split over K with every shape of the reduce, groups
with strides and per-group fragment tables, an extent on M (swizzle 2) and on K read on the device, leading dimensions
past the extent and base pointers off a 16-byte boundary.  tests/gemm_launch_grid.py holds the cases, the float64
reference and the host mirror of the plan; tests/test_gemm_launch_grid.py checks without a GPU that every cell is named.

Every call is held to four things: the plan it reports is the cell the table says it reaches (kernel, vec, vecC, table,
swizzle, splits, tiles, grid); every float of C it must not write -- rows at or beyond an extent, padding columns, the
gaps between groups -- keeps the canary bit for bit; everything it must not read holds 3e30, which no product survives;
and max |got - ref| / sum |a||b| < 2e-6 against float64 (modes 0, 6, 9; mode 3 is not fp32 and gets the rest).  On top, per
cell, the bitwise relation to the plainer call named in the test."""
import collections

import numpy as np
import pytest

import gemm_launch_grid as gl

pytestmark = pytest.mark.gpu

MODES = (0, 6, 9, 3)
CANARY_BITS = gl.CANARY.view(np.uint32)
REPORT = collections.OrderedDict()      # (cell, mode, kernel, vec, vecC, table, splits, swizzle) -> [calls, worst error]


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def engines(native):
    V, R, d, L, kind, nb = gl.ENGINE
    engs = {}
    for mode in MODES:
        e = native.Engine(V, R, d, L, kind, nb, max_edges=4, devtools=True)
        e.set_gemm_mode(mode)
        engs[mode] = e
    yield engs
    for e in engs.values():
        e.close()
    # one line per cell, mode and plan reached (pytest -s shows it): the plan and the worst normalised error
    for (cell, mode, kernel, vec, vecC, table, splits, swizzle), (n, err) in REPORT.items():
        print("gemm_launch_grid %-16s mode %d %-8s vec=%d vecC=%d table=%d splits=%-2d swizzle=%d calls=%-3d worst=%s"
              % (cell, mode, kernel, vec, vecC, table, splits, swizzle, n, "-" if err is None else "%.2e" % err))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def seed_of(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) % (2 ** 31)


def launch(eng, c, A, B, hide=True):
    a, b, cbuf = gl.build_operands(c, A, B, hide=hide)
    return eng.debug_gemm_call(a, b, cbuf, **gl.call_kwargs(c))


def check_call(c, mode, got, plan, A, B):
    """the four things of the module docstring; returns the per-group views of C"""
    tag = "%s mode %d" % (c["name"], mode)
    assert plan == gl.plan_mirror(c, mode), tag
    views, gaps = gl.product_views(c, got)
    assert (bits(got[gaps]) == CANARY_BITS).all(), "a gap between groups was written: " + tag
    worst = None
    for grp, ((mlim, klim), (ref, mag)) in enumerate(zip(gl.extents(c), gl.reference(c, A, B))):
        v = views[grp]
        assert (bits(v[mlim:]) == CANARY_BITS).all(), "rows at or beyond the extent were written: %s group %d" % (tag, grp)
        assert (bits(v[:, c["N"]:]) == CANARY_BITS).all(), "padding columns were written: %s group %d" % (tag, grp)
        prod = v[:mlim, :c["N"]].astype(np.float64)
        assert np.isfinite(prod).all(), "%s group %d" % (tag, grp)
        if klim == 0:
            assert not prod.any(), "an empty contraction is not exactly zero: %s group %d" % (tag, grp)
        live = mag > 0
        assert not prod[~live].any(), "%s group %d" % (tag, grp)
        if mode == 3 and live.any():
            # not fp32: hi.lo, lo.hi and mid.mid are dropped, each below 2^-18 |a||b| -- a bar a stray 3e30 cannot pass
            assert float((np.abs(prod - ref)[live] / mag[live]).max()) < 1e-4, "%s group %d" % (tag, grp)
        if mode != 3 and live.any():
            err = float((np.abs(prod - ref)[live] / mag[live]).max())
            print("%s group %d: %s vec=%d vecC=%d splits=%d swizzle=%d err %.3e" % (
                tag, grp, plan["kernel"], plan["vec"], plan["vecC"], plan["splits"], plan["swizzle"], err))
            assert err < gl.ACCURACY, "%s group %d: normalised error %.3e" % (tag, grp, err)
            worst = err if worst is None else max(worst, err)
    key = (c["cell"], mode, plan["kernel"], plan["vec"], plan["vecC"], plan["table"], plan["splits"], plan["swizzle"])
    n, w = REPORT.get(key, (0, None))
    REPORT[key] = [n + 1, worst if w is None else w if worst is None else max(w, worst)]
    return views


def plainer(c, **kw):
    out = dict(c)
    out.update(kw)
    return out


# ------------------------------------------------------------------ split over K
@pytest.mark.parametrize("mode", MODES)
def test_split_over_k(engines, mode):
    """2, 3, 8, 9 and 17 slices (the reduce's eight-wide loop, its tail, two rounds and a tail) on NN, NT and TN: the last
    slice a partial k-tile, exactly full, and K < 16 split_k where fewer slices exist than were asked -- the reported
    `splits` says which; N % 4 == 0 (k_splitk_reduce<4>), N = 5 or 127 (<1>), ldc > N with the canary in the padding."""
    for c in gl.cases_of("split"):
        A, B = gl.logical_operands(c, seed_of(c))
        got, plan = launch(engines[mode], c, A, B)
        s, K = c["split_k"], c["K"]
        assert plan["splits"] == (s if K > gl.BK * (s - 1) else gl.ceil_div(K, gl.BK)), c["name"]
        assert plan["slabs"] == (1 if plan["splits"] > 1 else 0) and plan["table"] == 0, c["name"]
        check_call(c, mode, got, plan, A, B)


def test_a_split_that_does_not_fit_the_slab_is_an_error(native, engines):
    """17 x 260 x 260 floats against the engine's 64 d^2: the general entry and the two older ones refuse an explicit
    split instead of lowering it, naming both numbers; the automatic choice may still fall back."""
    eng = engines[6]
    c = gl.case("too_large", "split", "TN", 260, 260, 272, split_k=17)
    need = 17 * 260 * 260
    assert need > gl.SLAB_FLOATS
    A, B = gl.logical_operands(c, 1)
    with pytest.raises(native.RgcnError) as e:
        launch(eng, c, A, B)
    assert str(need) in str(e.value) and str(gl.SLAB_FLOATS) in str(e.value), str(e.value)
    assert e.value.plan["splits"] == 17
    At = np.ascontiguousarray(A[0].T)
    for call in (lambda: eng.debug_gemm(At, B[0], trans_a=True, split_k=17),
                 lambda: eng.debug_gemm_time(At, B[0], trans_a=True, split_k=17, iters=1)):
        with pytest.raises(native.RgcnError) as e:
            call()
        assert str(need) in str(e.value) and str(gl.SLAB_FLOATS) in str(e.value), str(e.value)
    got = eng.debug_gemm(At, B[0], trans_a=True, split_k=0)
    ref = A[0].astype(np.float64) @ B[0].astype(np.float64)
    mag = np.abs(A[0]).astype(np.float64) @ np.abs(B[0]).astype(np.float64)
    assert float((np.abs(got - ref) / mag).max()) < gl.ACCURACY


# ------------------------------------------------------------------ groups
@pytest.mark.parametrize("mode", MODES)
def test_groups(engines, mode):
    """Two and three groups, strides larger than the operands with 3e30 in the gaps, without a table and with one fragment
    table per group on both pre-split-weight kernels, alone and together with a split: group g is bitwise the single-group
    call on group g's operands, canary padding included, and that call reports the same plan but for the grid -- and, where
    a gap is no multiple of 4 floats, but for the 16-byte accesses only the grouped call has to give up."""
    for c in gl.cases_of("groups"):
        A, B = gl.logical_operands(c, seed_of(c))
        got, plan = launch(engines[mode], c, A, B)
        views = check_call(c, mode, got, plan, A, B)
        aligned = all(c[k] % 4 == 0 for k in ("gap_a", "gap_b", "gap_c"))
        drop = ("grid_x", "grid_y") if aligned else ("grid_x", "grid_y", "vec", "vecC")
        for grp in range(c["groups"]):
            one = plainer(c, name=c["name"] + "_one", groups=1, gap_a=0, gap_b=0, gap_c=0)
            got1, plan1 = launch(engines[mode], one, A[grp:grp + 1], B[grp:grp + 1])
            assert {k: v for k, v in plan1.items() if k not in drop} == {k: v for k, v in plan.items() if k not in drop}, c["name"]
            assert plan1["grid_x"] == plan["grid_x"] and plan1["grid_y"] == 1, c["name"]
            np.testing.assert_array_equal(bits(views[grp]), bits(got1.reshape(views[grp].shape)),
                                          err_msg="%s mode %d group %d" % (c["name"], mode, grp))


# ------------------------------------------------------------------ extent on M
@pytest.mark.parametrize("mode", MODES)
def test_row_extent(engines, mode):
    """Swizzle 2: five groups whose row extents -- 0, 1, M - 3, M and one that leaves a whole 128-row panel out -- are read
    on the device from a table with limit_stride 3, on the fp32, staged and both pre-split-weight kernels.  Rows below the
    extent are bitwise the unlimited call's; rows at or beyond it and the padding columns keep the canary; the rows of A
    beyond the extent hold 3e30."""
    for c in gl.cases_of("row_extent"):
        A, B = gl.logical_operands(c, seed_of(c))
        got, plan = launch(engines[mode], c, A, B)
        assert plan["swizzle"] == 2 and plan["grid_x"] == 8 * plan["tiles_n"], c["name"]
        views = check_call(c, mode, got, plan, A, B)
        whole = plainer(c, name=c["name"] + "_unlimited", limit=None)
        gotw, planw = launch(engines[mode], whole, A, B)
        assert planw["swizzle"] == 1 and planw["kernel"] == plan["kernel"], c["name"]
        wviews = check_call(whole, mode, gotw, planw, A, B)
        for grp, (mlim, _) in enumerate(gl.extents(c)):
            np.testing.assert_array_equal(bits(views[grp][:mlim]), bits(wviews[grp][:mlim]),
                                          err_msg="%s mode %d group %d" % (c["name"], mode, grp))


@pytest.mark.parametrize("mode", MODES)
def test_row_extent_with_a_split_is_refused(native, engines, mode):
    """Tiles beyond a row extent write no slab and the reduce sums whole slabs: gemm_plan refuses the combination, nothing is
    launched and C keeps the caller's values (the entry copies C back only after a launch)."""
    for c in gl.REFUSED_CASES:
        A, B = gl.logical_operands(c, seed_of(c))
        with pytest.raises(native.RgcnError) as e:
            launch(engines[mode], c, A, B)
        assert e.value.status == 5 and gl.plan_mirror(c, mode) in str(e.value), str(e.value)      # RGCN_ERR_UNSUPPORTED
        assert e.value.plan["kernel"] == "none"


# ------------------------------------------------------------------ extent on K
@pytest.mark.parametrize("mode", MODES)
def test_depth_extent(engines, mode):
    """The depth of the contraction read on the device, two groups with different extents (one of them 0 in all but two
    cases), with and without a split over K; everything of A and B beyond the extent is 3e30.  Depth 0 gives exact zeros.
    Where the mirrored arithmetic says the device's slices are those of the plain call with K = extent, the product is
    bitwise that call's; the float64 bar holds always."""
    bitwise = 0
    for c in gl.cases_of("depth_extent"):
        A, B = gl.logical_operands(c, seed_of(c))
        got, plan = launch(engines[mode], c, A, B)
        assert plan["swizzle"] == 1 and plan["kernel"] != "w8", c["name"]
        views = check_call(c, mode, got, plan, A, B)
        g = gl.geometry(c)
        for grp, (_, klim) in enumerate(gl.extents(c)):
            if klim == 0 or not gl.slices_coincide(c["K"], c["split_k"], klim):
                continue
            # the same storage with K = extent: a k-contiguous operand keeps its leading dimension, the other loses rows
            short = plainer(c, name="%s_k%d" % (c["name"], klim), K=klim, groups=1, gap_a=0, gap_b=0, gap_c=0, limit=None,
                            limit_on_k=False, pad_a=c["pad_a"] + (c["K"] - klim if g["a_kc"] else 0),
                            pad_b=c["pad_b"] + (c["K"] - klim if g["b_kc"] else 0))
            gots, plans = launch(engines[mode], short, A[grp:grp + 1, :, :klim], B[grp:grp + 1, :klim])
            sviews = check_call(short, mode, gots, plans, A[grp:grp + 1, :, :klim], B[grp:grp + 1, :klim])
            np.testing.assert_array_equal(bits(views[grp]), bits(sviews[0]), err_msg="%s mode %d group %d" % (c["name"], mode, grp))
            bitwise += 1
    assert bitwise >= 8


def test_depth_extent_off_a_multiple_of_4_needs_dword_loads(native, engines):
    """16-byte loads of a k-contiguous operand take their four k all or nothing, and the plan cannot see an extent that
    lives on the device (GemmBatch::limit_on_k): the entry refuses such a call instead of reading past the extent."""
    c = gl.case("depth_77_vec", "depth_extent", "NN", 129, 132, 120, groups=2, gap_a=8, gap_b=8, gap_c=4, limit=(77, 0),
                limit_on_k=True)
    assert gl.plan_mirror(c, 6)["vec"] == 1
    A, B = gl.logical_operands(c, 3)
    with pytest.raises(native.RgcnError) as e:
        launch(engines[6], c, A, B)
    assert e.value.status == 1 and "multiple of 4" in str(e.value)


# ------------------------------------------------------------------ leading dimensions and alignment
@pytest.mark.parametrize("mode", MODES)
def test_leading_dimensions_and_alignment(engines, mode):
    """lda, ldb, ldc four floats past the extent: vec and vecC stay 1.  lda = K + 1 with K % 4 != 0, and each base pointer
    one float off a 16-byte boundary: vec resp. vecC drops to 0 and a fragment table is ignored where gemm_plan says so (a
    misaligned B behind its table does not matter).  What the plan must answer is pinned on the host by
    test_gemm_launch_grid.py and compared in check_call; padding and canaries stay intact; and the product is bitwise the
    contiguous, aligned call's -- how an operand is loaded and stored changes no arithmetic."""
    for cell in ("ld_plus_4", "ld_plus_1", "offset_a", "offset_b", "offset_c"):
        for c in gl.cases_of(cell):
            A, B = gl.logical_operands(c, seed_of(c))
            got, plan = launch(engines[mode], c, A, B)
            views = check_call(c, mode, got, plan, A, B)
            base = plainer(c, name=c["name"] + "_base", pad_a=0, pad_b=0, pad_c=0, off_a=0, off_b=0, off_c=0)
            gotb, planb = launch(engines[mode], base, A, B)
            bviews = check_call(base, mode, gotb, planb, A, B)
            assert planb["splits"] == plan["splits"], c["name"]
            np.testing.assert_array_equal(bits(views[0][:, :c["N"]]), bits(bviews[0]), err_msg="%s mode %d" % (c["name"], mode))
