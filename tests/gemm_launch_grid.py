"""The launch forms of the dense contractions (csrc/gemm_plan.h, gemm_f32.hip, gemm_bf16x3.hip, gemm_bf16x3_w8.hip) as a
table of small calls for tests/test_gpu_gemm_launch_grid.py, with what a test needs to hold a call to account on the host:

  plan_split / device_slices   the split arithmetic of gemm_plan() and its device-side recomputation under an extent on K
  plan_mirror                  the cell of the decision table a call must reach (kernel, vec, vecC, table, swizzle, splits)
  build_operands               the strided host buffers: random asymmetric operands, SENTINEL wherever the call must not
                               read, CANARY wherever it must not write
  reference                    per group op(A)[:Mlim, :Klim] @ op(B)[:Klim, :] in float64, and sum |a||b| beside it

tests/test_gemm_launch_grid.py keeps the table honest without a GPU: every cell the grid promises is named by a case."""
import numpy as np

BK, BM, BN, WIDE_BN = 16, 128, 128, 256           # kGemmBK, kGemmBM, kGemmBN, kGemmWideBN
SENTINEL = np.float32(3e30)                       # finite, and large enough to wreck any product it enters
CANARY = np.float32(-77.25)
FORMS = {"NN": (True, False), "NT": (True, True), "TN": (False, False)}      # (a_kc, b_kc)
ENGINE = (16, 2, 128, 1, "block", 16)             # V, R, d, L, kind, nb of the devtools engine the grid runs on
SLAB_FLOATS = 64 * 128 * 128                      # its split-K slab: 64 d^2 (rgcn_api.hip create_impl)
SHAPES = (1, 5, 127, 129, 132, 260)               # M and N of every case come from here
ACCURACY = 2e-6                                   # max |got - ref| / sum |a||b|: the bar test_gpu_parity.py holds modes 0, 6, 9 to


def ceil_div(a, b):
    return -(-a // b)


def plan_split(K, split_k):
    """(splits, k_per_split) as gemm_plan() computes them"""
    want = 1 if split_k < 1 else split_k
    kps = ceil_div(K, want)
    kps = ceil_div(kps, BK) * BK
    kps = max(kps, BK)
    return (ceil_div(K, kps) if K > 0 else 1), kps


def plain_slices(K, split_k):
    """[ks, ke) of every slice of a call without an extent on K"""
    splits, kps = plan_split(K, split_k)
    return [(z * kps, max(z * kps, min(K, z * kps + kps))) for z in range(splits)]


def device_slices(K, split_k, extent):
    """[ks, ke) of every slice when the depth is read on the device (GemmBatch::limit_on_k): the kernels divide the ACTUAL
    depth over the plan's slice count"""
    splits, _ = plan_split(K, split_k)
    klim = min(K, max(extent, 0))
    per = ceil_div(klim, splits)
    kps = max(BK, ceil_div(per, BK) * BK)
    return [(z * kps, max(z * kps, min(klim, z * kps + kps))) for z in range(splits)]


def slices_coincide(K, split_k, extent):
    """the non-empty slices of the limited call are those of the plain call with K = extent: the same partial sums are
    added in the same order (empty slices add +0), so the two products are bitwise equal"""
    live = lambda s: [x for x in s if x[1] > x[0]]
    return live(device_slices(K, split_k, extent)) == live(plain_slices(extent, split_k))


def case(name, cell, form, M, N, K, **kw):
    """pad_*: leading dimension minus the contiguous extent.  gap_*: floats between one group's operand and the next.
    limit: per-group extents (rows, or depth with limit_on_k), read on the device.  table: None, or which pre-split-weight
    kernel the call asks for ("presplit": knob 0, "w8": knob 3, both with a fragment table per group).  off_*: floats added
    to the 16-byte-aligned device base."""
    c = dict(name=name, cell=cell, form=form, M=M, N=N, K=K, pad_a=0, pad_b=0, pad_c=0, split_k=1, groups=1, gap_a=0, gap_b=0,
             gap_c=0, limit=None, limit_stride=1, limit_on_k=False, table=None, off_a=0, off_b=0, off_c=0)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    return c


def geometry(c):
    """leading dimensions, rows and group strides of the three buffers"""
    a_kc, b_kc = FORMS[c["form"]]
    M, N, K = c["M"], c["N"], c["K"]
    g = dict(a_kc=a_kc, b_kc=b_kc)
    g["rows_a"], g["cols_a"] = (M, K) if a_kc else (K, M)
    g["rows_b"], g["cols_b"] = (N, K) if b_kc else (K, N)
    g["lda"], g["ldb"], g["ldc"] = g["cols_a"] + c["pad_a"], g["cols_b"] + c["pad_b"], N + c["pad_c"]
    multi = c["groups"] > 1
    g["strideA"] = g["rows_a"] * g["lda"] + c["gap_a"] if multi else 0
    g["strideB"] = g["rows_b"] * g["ldb"] + c["gap_b"] if multi else 0
    g["strideC"] = M * g["ldc"] + c["gap_c"] if multi else 0
    return g


def extents(c):
    """(Mlim, Klim) of every group"""
    out = []
    for g in range(c["groups"]):
        n = None if c["limit"] is None else c["limit"][g]
        out.append((c["M"] if n is None or c["limit_on_k"] else n, c["K"] if n is None or not c["limit_on_k"] else n))
    return out


def limit_array(c):
    """the device-side extent table: group g's at [g * limit_stride], junk between"""
    if c["limit"] is None:
        return None
    lim = np.full((c["groups"] - 1) * c["limit_stride"] + 1, 10 ** 6, dtype=np.int32)
    lim[::c["limit_stride"]] = c["limit"]
    return lim


def vec_ok(offset, ld, extent):
    return offset % 4 == 0 and ld % 4 == 0 and extent % 4 == 0 and extent >= 4


def reduce_width(c):
    """VEC of k_splitk_reduce (gemm_run), 0 when the call has no split"""
    g = geometry(c)
    if plan_split(c["K"], c["split_k"])[0] == 1:
        return 0
    return 4 if c["N"] % 4 == 0 and g["ldc"] % 4 == 0 and c["off_c"] % 4 == 0 and g["strideC"] % 4 == 0 else 1


def plan_mirror(c, mode):
    """What gemm_plan() answers for the case (the fields rgcn_debug_gemm_call reports), or the refusal as a string.
    The knob is 0 or 3 in every case, so the tile-count heuristic of a wide request never decides."""
    g = geometry(c)
    a_kc, b_kc, M, N, K = g["a_kc"], g["b_kc"], c["M"], c["N"], c["K"]
    row_limit = c["limit"] is not None and not c["limit_on_k"]
    if row_limit and c["split_k"] > 1:
        return "gemm: a row limit cannot be combined with a split over K"
    nn = a_kc and not b_kc
    has_table = c["table"] is not None
    b_unread = has_table and nn and mode != 0 and c["split_k"] <= 1
    vec = (vec_ok(c["off_a"], g["lda"], g["cols_a"]) and (b_unread or vec_ok(c["off_b"], g["ldb"], g["cols_b"])) and
           g["strideA"] % 4 == 0 and (b_unread or g["strideB"] % 4 == 0))
    splits, kps = plan_split(K, c["split_k"])
    slabs = splits > 1
    ldc = N if slabs else g["ldc"]
    vecC = ((slabs or c["off_c"] % 4 == 0) and ldc % 4 == 0 and N % 4 == 0 and
            (slabs or c["groups"] <= 1 or g["strideC"] % 4 == 0))
    kernel, table, bn = "f32", False, BN
    if mode != 0:
        table = has_table and splits == 1 and a_kc and vec
        w8 = table and not c["limit_on_k"] and mode != 3 and c["table"] == "w8"
        kernel = "w8" if w8 else "presplit" if table else "staged"
        bn = WIDE_BN if w8 else BN
    swizzle = 2 if row_limit else 1
    tiles_m, tiles_n = ceil_div(M, BM), ceil_div(N, bn)
    grid_x = ceil_div(tiles_m, 8) * 8 * tiles_n if swizzle == 2 else tiles_m * tiles_n * splits
    return dict(kernel=kernel, terms={0: 0, 3: 3, 6: 6, 9: 9}[mode], vec=int(vec), vecC=int(vecC), table=int(table), prologue=0,
                swizzle=swizzle, splits=splits, k_per_split=kps, slabs=int(slabs), ldc=ldc, tiles_m=tiles_m, tiles_n=tiles_n,
                grid_x=grid_x, grid_y=c["groups"])


def call_kwargs(c):
    """the arguments of Engine.debug_gemm_call beside the three buffers"""
    g = geometry(c)
    return dict(M=c["M"], N=c["N"], K=c["K"], a_kc=g["a_kc"], b_kc=g["b_kc"], lda=g["lda"], ldb=g["ldb"], ldc=g["ldc"],
                split_k=c["split_k"], groups=c["groups"], strideA=g["strideA"], strideB=g["strideB"], strideC=g["strideC"],
                limit=limit_array(c), limit_stride=c["limit_stride"], limit_on_k=c["limit_on_k"],
                presplit_b=c["table"] is not None, wide=1 if c["table"] == "w8" else 0, w8_knob=3 if c["table"] == "w8" else 0,
                a_offset=c["off_a"], b_offset=c["off_b"], c_offset=c["off_c"])


def logical_operands(c, seed):
    """per group op(A) [M, K] and op(B) [K, N], float32: asymmetric, B spread over magnitudes"""
    rng = np.random.RandomState(seed)
    M, N, K = c["M"], c["N"], c["K"]
    A = rng.randn(c["groups"], M, K).astype(np.float32)
    B = (rng.randn(c["groups"], K, N) * np.exp(rng.uniform(-6, 6, (c["groups"], K, N)))).astype(np.float32)
    return A, B


def build_operands(c, A, B, hide=True):
    """The flat host buffers of the call for logical operands A [groups, M, K], B [groups, K, N].  SENTINEL: the padding
    columns, the gaps between groups and -- hide -- the rows of A beyond a row extent and everything of A and B beyond an
    extent on K.  C is CANARY throughout."""
    g = geometry(c)
    n = c["groups"]
    a = np.full((n - 1) * g["strideA"] + g["rows_a"] * g["lda"], SENTINEL, dtype=np.float32)
    b = np.full((n - 1) * g["strideB"] + g["rows_b"] * g["ldb"], SENTINEL, dtype=np.float32)
    for grp, (mlim, klim) in enumerate(extents(c)):
        Ag, Bg = A[grp].copy(), B[grp].copy()
        if hide:
            Ag[mlim:, :] = SENTINEL
            Ag[:, klim:] = SENTINEL
            Bg[klim:, :] = SENTINEL
        av = a[grp * g["strideA"]: grp * g["strideA"] + g["rows_a"] * g["lda"]].reshape(g["rows_a"], g["lda"])
        bv = b[grp * g["strideB"]: grp * g["strideB"] + g["rows_b"] * g["ldb"]].reshape(g["rows_b"], g["ldb"])
        av[:, :g["cols_a"]] = Ag if g["a_kc"] else Ag.T
        bv[:, :g["cols_b"]] = Bg.T if g["b_kc"] else Bg
    cbuf = np.full((n - 1) * g["strideC"] + c["M"] * g["ldc"], CANARY, dtype=np.float32)
    return a, b, cbuf


def product_views(c, cflat):
    """[group g's M x ldc view of the flat C buffer], and a mask of the floats no group owns (the gaps)"""
    g = geometry(c)
    owned = np.zeros(cflat.shape, dtype=bool)
    views = []
    for grp in range(c["groups"]):
        lo = grp * g["strideC"]
        views.append(cflat[lo: lo + c["M"] * g["ldc"]].reshape(c["M"], g["ldc"]))
        owned[lo: lo + c["M"] * g["ldc"]] = True
    return views, ~owned


def reference(c, A, B):
    """per group (ref, mag) in float64: op(A)[:Mlim, :Klim] @ op(B)[:Klim, :] and the same product of absolute values"""
    out = []
    for grp, (mlim, klim) in enumerate(extents(c)):
        a = A[grp, :mlim, :klim].astype(np.float64)
        b = B[grp, :klim, :].astype(np.float64)
        out.append((a @ b, np.abs(a) @ np.abs(b)))
    return out


# ------------------------------------------------------------------ the table
SPLIT_COUNTS = (2, 3, 8, 9, 17)          # the reduce's eight-wide loop (8), its tail (2, 3, 9), two rounds and a tail (17)
TABLES = (None, "presplit", "w8")


def _split_cases():
    # per split count: (M, N) of the three K choices; N % 4 == 0 -> k_splitk_reduce<4>, N = 5 or 127 -> k_splitk_reduce<1>
    shapes = {2: ((260, 132), (127, 5), (129, 260)), 3: ((129, 260), (132, 5), (5, 127)), 8: ((132, 260), (129, 5), (1, 132)),
              9: ((260, 260), (127, 5), (129, 127)), 17: ((129, 132), (260, 5), (127, 260))}
    out = []
    for s in SPLIT_COUNTS:
        k_partial = 32 * s - 5 if s <= 3 else 16 * s - 3      # the last slice ends inside a k-tile (two tiles a slice at 2, 3)
        k_full = 16 * s                                        # every slice exactly one k-tile
        k_few = 16 * s - 20                                    # K < 16 s: fewer slices than asked (none at s = 2)
        for form in FORMS:
            (m0, n0), (m1, n1), (m2, n2) = shapes[s]
            out.append(case("split%d_%s_partial" % (s, form), "split", form, m0, n0, k_partial, split_k=s, pad_c=4))
            out.append(case("split%d_%s_full" % (s, form), "split", form, m1, n1, k_full, split_k=s, pad_c=3))
            out.append(case("split%d_%s_few" % (s, form), "split", form, m2, n2, k_few, split_k=s))
    return out


def _group_cases():
    out = []
    for table in TABLES:
        t = table or "staged"
        out.append(case("groups2_NN_%s" % t, "groups", "NN", 129, 132, 36, groups=2, gap_a=8, gap_b=12, gap_c=4, table=table))
        out.append(case("groups3_NT_%s" % t, "groups", "NT", 127, 260, 52, groups=3, gap_a=4, gap_b=8, gap_c=12, table=table))
        out.append(case("groups2_NN_n260_%s" % t, "groups", "NN", 260, 260, 20, groups=2, gap_a=4, gap_b=4, gap_c=8, pad_c=4,
                        table=table))
    # odd gaps: dword loads; an odd gap between the products: dword stores although N and ldc would allow 16 bytes
    out.append(case("groups3_NN_odd_gaps", "groups", "NN", 132, 132, 40, groups=3, gap_a=5, gap_b=3, gap_c=8))
    out.append(case("groups2_NT_odd_c_gap", "groups", "NT", 129, 132, 24, groups=2, gap_a=4, gap_b=4, gap_c=5))
    out.append(case("groups2_TN", "groups", "TN", 132, 129, 33, groups=2, gap_a=8, gap_b=7, gap_c=6))
    # groups and a split over K: every group its own slabs (N % 4 == 0 and N = 5: both reduce kernels index by group)
    out.append(case("groups3_TN_split3", "groups", "TN", 132, 5, 77, groups=3, split_k=3, gap_a=8, gap_b=5, gap_c=7))
    out.append(case("groups2_TN_split9", "groups", "TN", 129, 132, 141, groups=2, split_k=9, gap_a=4, gap_b=8, gap_c=12, pad_c=4))
    out.append(case("groups2_NN_split2", "groups", "NN", 127, 260, 59, groups=2, split_k=2, gap_a=3, gap_b=4, gap_c=4))
    return out


def _row_extent_cases():
    # one group per extent: 0, 1, M - 3, M and one that leaves a whole 128-row panel out; the table of extents has
    # limit_stride 3
    out = []
    for M, N, K, lims in ((129, 132, 40, (0, 1, 126, 129, 100)), (260, 5, 24, (0, 1, 257, 260, 129))):
        for form in FORMS:
            for table in TABLES if form != "TN" else (None,):
                out.append(case("rows_%s_m%d_%s" % (form, M, table or "staged"), "row_extent", form, M, N, K, groups=5,
                                gap_a=8, gap_b=4, gap_c=8, pad_c=4, limit=lims, limit_stride=3, table=table))
    return out


def _depth_extent_cases():
    out = []
    # k-contiguous operands with 16-byte loads: extents that are multiples of 4 (gemm_plan.h GemmBatch::limit_on_k)
    for form in ("NN", "NT"):
        out.append(case("depth_%s" % form, "depth_extent", form, 129, 132, 120, groups=2, gap_a=8, gap_b=8, gap_c=4,
                        limit=(76, 0), limit_on_k=True))
        out.append(case("depth_%s_split3" % form, "depth_extent", form, 132, 260, 120, groups=2, gap_a=8, gap_b=8, gap_c=4,
                        split_k=3, limit=(0, 76), limit_stride=2, limit_on_k=True, pad_c=4))
        # dword loads (lda = K + 1): any extent
        out.append(case("depth_%s_dword" % form, "depth_extent", form, 127, 5, 120, groups=2, gap_a=3, gap_b=4, gap_c=4,
                        pad_a=1, limit=(77, 0), limit_on_k=True))
    out.append(case("depth_NN_presplit", "depth_extent", "NN", 260, 132, 120, groups=2, gap_a=8, gap_b=8, gap_c=4,
                    limit=(76, 0), limit_on_k=True, table="presplit"))
    out.append(case("depth_NN_w8_asked", "depth_extent", "NN", 129, 260, 64, groups=2, gap_a=8, gap_b=8, gap_c=4,
                    limit=(0, 36), limit_on_k=True, table="w8"))      # (never the eight-wavefront kernel: it reads a row limit)
    # the form of the one call site (units_product_dw): any extent
    out.append(case("depth_TN", "depth_extent", "TN", 132, 129, 120, groups=2, gap_a=8, gap_b=4, gap_c=8,
                    limit=(77, 0), limit_on_k=True))
    out.append(case("depth_TN_split3", "depth_extent", "TN", 260, 132, 120, groups=2, gap_a=8, gap_b=4, gap_c=8, split_k=3,
                    limit=(0, 77), limit_on_k=True, pad_c=4))
    out.append(case("depth_TN_split8", "depth_extent", "TN", 129, 5, 120, groups=2, gap_a=8, gap_b=4, gap_c=8, split_k=8,
                    limit=(20, 120), limit_on_k=True))
    # fewer slices than asked (K = 100, 5 asked: 4 of 32), and an extent whose slices are NOT those of the plain call
    out.append(case("depth_TN_split5_other_slices", "depth_extent", "TN", 127, 132, 100, groups=2, gap_a=8, gap_b=4, gap_c=8,
                    split_k=5, limit=(68, 96), limit_on_k=True))
    return out


def _layout_cases():
    out = []
    # leading dimensions four floats past the extent: 16-byte loads and stores stay
    for form, M in (("NN", 129), ("NT", 127), ("TN", 132)):
        for table in TABLES if form != "TN" else (None,):
            out.append(case("ld4_%s_%s" % (form, table or "staged"), "ld_plus_4", form, M, 132, 36, pad_a=4, pad_b=4, pad_c=4,
                            table=table))
        out.append(case("ld4_%s_split3" % form, "ld_plus_4", form, M if form == "TN" else 260, 260, 92, pad_a=4, pad_b=4,
                        pad_c=4, split_k=3))
    # lda = K + 1 with K % 4 != 0 (TN: lda = M + 1, M % 4 != 0)
    for form in FORMS:
        out.append(case("ld1_%s" % form, "ld_plus_1", form, 129, 132, 37, pad_a=1, table="presplit" if form != "TN" else None))
    # each base pointer one float past a 16-byte boundary; the table is asked for wherever the form could take it
    for form, M in (("NN", 129), ("NT", 260), ("TN", 132)):
        table = "w8" if form != "TN" else None
        out.append(case("offA_%s" % form, "offset_a", form, M, 132, 36, off_a=1, table=table, pad_c=4))
        out.append(case("offB_%s" % form, "offset_b", form, M, 132, 36, off_b=1, table=table, pad_c=4))
        out.append(case("offC_%s" % form, "offset_c", form, M, 132, 36, off_c=1, table=table, pad_c=4))
        out.append(case("offC_%s_split3" % form, "offset_c", form, M, 132, 92, off_c=1, split_k=3, pad_c=4))
    out.append(case("offABC_NN_n5", "offset_a", "NN", 127, 5, 20, off_a=3, off_b=2, off_c=1, table="presplit"))
    return out


CASES = {c["name"]: c for c in _split_cases() + _group_cases() + _row_extent_cases() + _depth_extent_cases() + _layout_cases()}

# a row limit together with a split over K: gemm_plan refuses it (the reduce sums whole slabs)
REFUSED_CASES = [case("rows_split3_refused", "row_extent_split", "TN", 129, 132, 92, split_k=3, limit=(100,)),
                 case("rows_split2_groups_refused", "row_extent_split", "NN", 132, 132, 64, split_k=2, groups=2, gap_a=4,
                      gap_b=4, gap_c=4, limit=(1, 132))]


def cases_of(cell):
    return [c for c in CASES.values() if c["cell"] == cell]
