"""Highway skip connections, IncidenceNormalization=local and the output transform at FULL-GRAPH scale.

Above 65,536 messages the block encoder on one GPU runs in another regime (tests/giant_grid.py): rows of more than 2048
slots are summed piece by piece (k_combine / k_block_rows pieces, k_combine_giant_finish, k_colsum_giant_rows), the relation
chunk grows, and bwd_block_rows (rgcn_schedule.hip) takes its third branch -- the relation-weight kernels on side stream 0
from the start of the layer, dw_pending, a join before the next layer.  Every full-graph evaluation pass runs there.  The
three features below were merged after tests/giant_grid.py was written, and each changes what the block layer's epilogue
does:

  highway (highway.hip)    the layer writes N_l into hw_N[l]; the backward epilogue leaves the raw dH (no gate, no dropout
                           copy, no column sums); gemm_highway_dw shares side stream 1 and the slabs with dW_self;
                           bwd_highway_open runs ahead of the dw_pending join; db_emb's partials come from k_highway_join
  local norms              d_norm / s_norm of k_build_msgs along the pieces of a cut row
  output transform         output_backward ahead of a full-graph backward pass; dcodes is [V, code_dim]

FULLGRAPH_GRID is the smallest shape that reaches the regime with each of them and with all three.  The functions below
build a case's graph and inputs, restate the encoder in float64 (and once more in plain float32) out of the features' own
reference modules, and hold an engine's or a restatement's tensors to the features' own bars.
tests/test_fullgraph_grid.py keeps the table honest without a GPU; tests/test_gpu_fullgraph_grid.py runs it.
"""
import numpy as np

import giant_grid as gg
import helpers
import highway_reference as hr
import kernel_grid as kg
import local_norm_reference as lnr
import output_transform_reference as otr

FWD_ATOL = 1e-4        # test_gpu_highway.py's, test_gpu_local_norm.py's and test_gpu_output_transform.py's: one figure
KEEP = 0.8
HUB_LOCAL, HUB_LOST = 5, 6      # the 4097-slot row fg_local relabels; the 6000-slot row whose last piece item 8 drops


def _case(name, seed, nb=4, sd=5, L=2, kind="block", skip="none", norm="intended", code_dim=0, relabel=False):
    """seed: one under which the graph's only long rows are the seven hubs (tests/test_fullgraph_grid.py checks)"""
    return dict(name=name, kind=kind, V=gg.V_STD, R=gg.R_GIANT, d=nb * sd, L=L, nb=nb, E=gg.E_STD, hubs=gg.HUBS, seed=seed,
                max_edges=gg.E_STD, drop_free_edge=False, skip=skip, norm=norm, code_dim=code_dim, relabel=relabel)


FULLGRAPH_GRID = [
    # giant finish with the highway epilogue, forward (relu into hw_N) and backward (no gate, no dropout copy); the third
    # branch of bwd_block_rows under highway; db_emb from highway_join while the cut is on
    _case("fg_highway", 8001, skip="highway"),
    # dbuf / dsbuf / hw_dz ping-pong and the dw_pending join across three layers
    _case("fg_highway_L3", 8002, skip="highway", L=3),
    # highway CL = 256 with GW 32 and the piece loop's second column chunk; split-K of gemm_highway_dw and gemm_self_dw
    # sharing slabs at K = 3000
    _case("fg_highway_wide", 8003, skip="highway", nb=129, sd=4),
    # the scalar forms of the finish kernel and of the highway kernels together
    _case("fg_highway_vec1", 8004, skip="highway", nb=3, sd=3),
    # the full-graph relation chunk (96) under a highway context; the basis kind is never cut
    _case("fg_highway_basis", 8005, skip="highway", kind="basis", nb=2, sd=10),
    # d_norm / s_norm along pieces: the 4097-slot row is two runs of one directed relation each
    _case("fg_local", 8006, norm="local", relabel=True),
    # output_backward ahead of a full-graph backward pass
    _case("fg_out", 8007, code_dim=8),
    _case("fg_all", 8008, skip="highway", norm="local", relabel=True, code_dim=8),
]
FULLGRAPH_CASES = {c["name"]: c for c in FULLGRAPH_GRID}
EVAL_CASES = ("fg_highway", "fg_local", "fg_all")
FORM_CASES = ("fg_highway", "fg_local", "fg_out")
LOST_PIECE_CASES = ("fg_highway", "fg_all")
# what each row of the table says its graph holds: the slot counts of the rows the engine cuts
GIANT_ROWS = {c["name"]: [] if c["kind"] == "basis" else [2049, 4096, 4097, 6000] for c in FULLGRAPH_GRID}


# ----------------------------------------------------------------------------- graphs
def relabel_relation(case):
    """The one relation fg_local's 4097-slot row is relabelled to (any will do; not 0 and not R - 1)."""
    return case["R"] // 2


def case_triples(case):
    """giant_grid's standard graph; relabel: every edge at vertex HUB_LOCAL carries one relation, so that row is two runs
    of one directed relation each -- 2049 arriving edges (norm 1 / 2049 under `local`), then 2048 leaving ones (1 / 2048)."""
    t = gg.giant_triples(case)
    if case["relabel"]:
        t = np.array(t)
        t[(t[:, 0] == HUB_LOCAL) | (t[:, 2] == HUB_LOCAL), 1] = relabel_relation(case)
    return np.ascontiguousarray(t)


def small_triples(case):
    """kernel_grid's 3,000-edge graph (rows of 33, 100 and 400 slots) at the case's V and R: minibatch branch, cut off"""
    return kg.grid_triples(dict(V=case["V"], R=case["R"], E=kg.E_GRID, hubs=(33, 100, 400), seed=case["seed"] + 1))


def row_slot_order(triples, R, v):
    """Incidence ids of row v in slot order (graph_prep.hip, k_keys: incidence i < E is edge i seen from its object,
    i >= E edge i - E seen from its subject; a row's slots are ordered by directed relation -- r arriving, R + r leaving
    -- ties by incidence id).  Returns (incidence ids, directed relations)."""
    t = np.asarray(triples).reshape(-1, 3)
    E = len(t)
    inc = np.concatenate([np.flatnonzero(t[:, 2] == v), E + np.flatnonzero(t[:, 0] == v)])
    rel2 = np.where(inc < E, t[inc % E, 1], R + t[inc % E, 1])
    order = np.lexsort((inc, rel2))
    return inc[order], rel2[order]


def runs_of(rel2):
    """lengths of the runs of equal directed relation along a row's slots"""
    cut = np.flatnonzero(np.diff(rel2)) + 1
    return np.diff(np.concatenate([[0], cut, [len(rel2)]])).tolist()


# ----------------------------------------------------------------------------- inputs
def case_inputs(case):
    """The case with params, triples, masks (train mode, keep 0.8) and dcodes: highway_reference.make_case's for a highway
    case, helpers.make_case's otherwise; under code_dim c the output layer's W_out [d, c], b_out [c], W_relation [V, c] and
    an upstream gradient [V, c] on top (output_transform_reference.make_case's scales)."""
    c = dict(case)
    V, R, d, L, kind, nb = (c[k] for k in ("V", "R", "d", "L", "kind", "nb"))
    c["triples"] = case_triples(case)
    if c["skip"] == "highway":
        h = hr.make_case(V, R, d, L, kind, nb, c["triples"], seed=c["seed"], keep=KEEP)
        c["params"], c["masks"], c["dcodes"] = h["params"], h["masks"], h["dcodes"]
    else:
        c["params"], _, c["masks"], c["dcodes"] = helpers.make_case(V, R, d, L, kind, nb, 0, seed=c["seed"], keep=KEEP)
    if c["code_dim"]:
        from relationprediction_amd.common.shared_functions import glorot_variance
        cd, rng = c["code_dim"], np.random.RandomState(c["seed"] + 5)
        c["params"]["W_out"] = rng.normal(0, glorot_variance([d, cd]), size=(d, cd)).astype(np.float32)
        c["params"]["b_out"] = (rng.randn(cd) * 0.3).astype(np.float32)
        c["params"]["W_relation"] = rng.randn(V, cd).astype(np.float32)
        c["dcodes"] = (rng.randn(V, cd) * 1e-1).astype(np.float32)
    c["keep"] = KEEP
    return c


def weight_names(case):
    """rgcn_param_info names of the case's context: the stack's, the output layer's [W_out, b_out] under W_relation"""
    import oracle
    names = hr.weight_names(case["kind"], case["L"]) if case["skip"] == "highway" else oracle.weight_names(case["kind"], case["L"])
    return names[:-1] + (["W_out", "b_out"] if case["code_dim"] else []) + ["W_relation"]


def unused_bias(name):
    """b<l>: the layers' own biases, which the block and basis layers never add -- their gradient is all zeros"""
    return name[0] == "b" and name[1:].isdigit()


# ----------------------------------------------------------------------------- the restatement, float64 and float32
def case_norms(c, triples, dtype=np.float64):
    """(n_f, n_b) per edge.  float64: the exact rational's rounding; float32: what the device computes, float32(1) /
    float32(count).  None: the highway restatement's own `intended` norms (its chunked float64 layers)."""
    if c["norm"] == "intended" and c["skip"] == "highway":
        return None
    if dtype == np.float64:
        return lnr.norms(triples, c["V"], c["norm"])
    n_f, n_b = lnr.message_norms_f32(triples, c["V"], c["norm"])
    return np.asarray(n_f, dtype=np.float32), np.asarray(n_b, dtype=np.float32)


def reference_forward(c, masks=None, mode="train", dtype=np.float64, triples=None):
    """{"H": [H0..HL], "N": [None, N1..NL], "T": [None, T1..TL] (highway cases), "codes": [V, c] (code_dim cases)}"""
    triples = c["triples"] if triples is None else triples
    masks = c["masks"] if masks is None and mode == "train" else masks
    kind, V, L = c["kind"], c["V"], c["L"]
    norms = case_norms(c, triples, dtype)
    out = {}
    if c["skip"] == "highway":
        if dtype == np.float64:
            out["H"], out["N"], out["T"] = hr.forward(kind, c["params"], triples, V, L, mode=mode, keep=KEEP, masks=masks, norms=norms)
        else:
            out["H"], out["N"], out["T"] = hr.forward_float32(kind, c["params"], triples, V, L, mode=mode, keep=KEEP, masks=masks,
                                                              norms=norms)
    else:
        out["H"] = lnr.forward(kind, c["params"], triples, V, L, norms[0], norms[1], mode=mode, keep=KEEP, masks=masks, dtype=dtype)
    if c["code_dim"]:
        out["codes"] = otr.layer_forward(out["H"][L], c["params"]["W_out"], c["params"]["b_out"], dtype=dtype)
    return out


def reference_backward(c, acts, masks=None, mode="train", dtype=np.float64, triples=None):
    """Gradient of <dcodes, codes> with respect to every encoder parameter, evaluated AT the given activations (an
    engine's own H_l, N_l and T_l: its own relu gates)."""
    triples = c["triples"] if triples is None else triples
    masks = c["masks"] if masks is None and mode == "train" else masks
    kind, V, L = c["kind"], c["V"], c["L"]
    norms = case_norms(c, triples, dtype)
    top = np.asarray(c["dcodes"], dtype=dtype)
    extra = {}
    if c["code_dim"]:
        top, extra["W_out"], extra["b_out"] = otr.layer_backward(acts["H"][L], c["params"]["W_out"], c["dcodes"], dtype=dtype)
    stack = {k: v for k, v in c["params"].items() if k not in ("W_out", "b_out", "W_relation")}
    if c["skip"] == "highway":
        g = hr.backward(kind, stack, triples, V, L, acts["H"], acts["N"], acts["T"], top, mode=mode, keep=KEEP, masks=masks,
                        dtype=dtype, norms=norms)
    else:
        g = lnr.backward(kind, stack, triples, V, L, norms[0], norms[1], acts["H"], top, mode=mode, keep=KEEP, masks=masks,
                         dtype=dtype)
    g.update(extra)
    return g


def lost_piece_mirror(c, ref):
    """The float64 forward with the LAST piece of row HUB_LOST (6000 slots: 1904 of them) left out of N_1: what a finish
    kernel that dropped a row's last piece would produce.  Only N_1 is rewritten; nothing runs an altered kernel."""
    t, E, V = c["triples"], len(c["triples"]), c["V"]
    inc, _ = row_slot_order(t, c["R"], HUB_LOST)
    assert len(inc) == 6000 and gg.last_piece(len(inc)) == 1904 and c["L"] > 1
    norms = lnr.norms(t, V, c["norm"])
    p = {k: np.asarray(v, dtype=np.float64) for k, v in c["params"].items()}
    H0 = ref["H"][0]
    self_part = (H0[HUB_LOST] @ p["W_self1"]) * (np.asarray(c["masks"][0][HUB_LOST], dtype=np.float64) / KEEP)

    def row(slots):
        pre = self_part.copy()
        for tag, nrm, ids, col_in in (("f", norms[0], slots[slots < E], 0), ("b", norms[1], slots[slots >= E] - E, 2)):
            if len(ids):
                pre += (lnr._messages(c["kind"], 1, p, H0, t[ids, col_in], t[ids, 1], tag) * nrm[ids, None]).sum(axis=0)
        return np.maximum(pre, 0.0)

    # the bookkeeping above is right: all 6000 slots give the restatement's own row (to 1e-6: the chunked float64 layers
    # of an `intended` highway case take the float32 value of 1 / degree, lnr.norms the exact one)
    whole = row(inc)
    assert np.abs(whole - ref["N"][1][HUB_LOST]).max() <= 1e-6 * max(1.0, np.abs(whole).max())
    out = dict(ref)
    out["N"] = list(ref["N"])
    n1 = np.array(ref["N"][1])
    n1[HUB_LOST] = row(inc[:-gg.last_piece(len(inc))])
    out["N"][1] = n1
    return out, float(np.abs(n1[HUB_LOST] - whole).max())


# ----------------------------------------------------------------------------- the check
def compared_activations(c, acts):
    """(name, tensor) of everything item 1 compares in the forward pass"""
    L = c["L"]
    out = [("H%d" % l, acts["H"][l]) for l in range(L + 1)]
    if c["skip"] == "highway":
        out += [("N%d" % l, acts["N"][l]) for l in range(1, L + 1)] + [("T%d" % l, acts["T"][l]) for l in range(1, L + 1)]
    if c["code_dim"]:
        out.append(("codes", acts["codes"]))
    return out


def check_forward(c, acts, ref, tag=""):
    """The features' own forward bar: every activation within FWD_ATOL absolute of float64; no tensor all zeros.
    Returns the report lines `name max-abs (max / l2 of scale)`."""
    report = []
    for (name, got), (_, want) in zip(compared_activations(c, acts), compared_activations(c, ref)):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (tag, c["name"], name, got.shape, want.shape)
        assert np.isfinite(got).all(), "%s%s %s non-finite" % (tag, c["name"], name)
        assert np.abs(want).max() > 0 and np.abs(got).max() > 0, "%s%s %s is all zeros" % (tag, c["name"], name)
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst, l2 = helpers.error_against(want, got)
        report.append("%s %.2e (%.1e/%.1e)" % (name, err, worst, l2))
        assert err <= FWD_ATOL, "%s%s %s against float64: max abs err %.3e (scale %.3e)" % (
            tag, c["name"], name, err, float(np.abs(want).max()))
        if name[0] == "T":
            assert ((got >= 0) & (got <= 1)).all(), (tag, c["name"], name)
    return report


def check_gradients(c, grads, g64, tag=""):
    """The features' own gradient bar: helpers.assert_close with its defaults against the float64 reverse mode at the
    activations the gradients belong to; no tensor all zeros but the layers' unused biases."""
    names = weight_names(c)[:-1]
    assert set(g64) == set(names), sorted(set(g64) ^ set(names))
    report = []
    for n in names:
        worst, l2 = helpers.error_against(g64[n], grads[n])
        report.append("%s %.1e/%.1e" % (n, worst, l2))
        if unused_bias(n):
            assert not np.asarray(grads[n]).any() and not g64[n].any(), n
            continue
        assert np.abs(g64[n]).max() > 0 and np.abs(grads[n]).max() > 0, "%s%s %s is all zeros" % (tag, c["name"], n)
        helpers.assert_close(grads[n], g64[n], name="%s%s %s" % (tag, c["name"], n))
    return report


def check_against_float64(c, acts, grads, ref, g64, tag=""):
    """Item 1's comparison, of an engine's step or of the float32 restatement: (forward report, gradient report)"""
    fwd = check_forward(c, acts, ref, tag)
    return fwd, (check_gradients(c, grads, g64, tag) if grads is not None else [])
