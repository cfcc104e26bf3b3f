"""The giant-row cut on the GPU (tests/giant_grid.py's table) against float64: every block size, both vector widths,
every group width, last pieces of 1 / 2048 / 1904 slots, the longest uncut row, more giant rows than the finish kernel
has workgroups, the 2E = 65,536 | 65,538 switch, one context alternating between a cut and an uncut graph, and the
column-sum fallback.  The bars are test_gpu_parity.py::test_float64_tie_break's, unchanged: forward within 2e-5 of the
layer's scale (l2 5e-6); every gradient against the float64 reverse mode of the engine's own forward within 5e-6 of
scale (l2 2e-6) and no worse than 4 x the fp32 oracle's own l2 distance + 1e-7.  On these graphs the fp32 oracle alone
sits at most 5.2e-7 / 2.9e-7 from float64 in the forward pass (1.6e-6 / 4.0e-7 with the as-executed normalisation) and
3.1e-6 / 1.7e-6 in the gradients (b_emb, its 3,000-term fp32 column sums; every other gradient at most 1.6e-6 / 8.6e-7);
the engine at most 9.3e-7 / 4.8e-7 and 1.5e-6 / 1.1e-6.  (Tried once: with k_ptrs' piece count rounded down, a fault both
forms share, the bitwise comparisons below all pass and every float64 case with the cut on fails.)"""
import functools

import numpy as np
import pytest

import oracle
import helpers
import giant_grid as gg
import kernel_grid as kg
from test_gpu_parity import _single_pass_equals_two_kernel_form

pytestmark = pytest.mark.gpu

FWD_MAX, FWD_L2 = 2e-5, 5e-6          # test_float64_tie_break's bars
GRAD_MAX, GRAD_L2 = 5e-6, 2e-6
LOST_PIECE_CASE, LOST_PIECE_ROW, LOST_PIECE_TO = "giant_sd5_nb4", 3, 8


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@functools.lru_cache(maxsize=None)
def case_of(name):
    """The case with its inputs, built once per module and never written to."""
    c = dict(gg.GIANT_CASES[name])
    c["params"], c["triples"], c["masks"], c["dcodes"] = gg.giant_inputs(c)
    for a in [c["triples"], c["dcodes"]] + list(c["masks"]) + list(c["params"].values()):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def forward64(name, norm="intended", mode="train"):
    c = case_of(name)
    with helpers.oracle_float64():
        p64 = {k: np.asarray(v, dtype=np.float64) for k, v in c["params"].items()}
        acts = oracle.encoder_forward(p64, c["triples"], c["V"], c["L"], c["kind"], mode=mode, keep_prob=0.8,
                                      dropout_masks=c["masks"], norm_mode=norm)
    for a in acts:
        a.setflags(write=False)
    return acts


def step(native, c, triples=None, norm="intended", train=True, max_edges=None, backward=True, eng=None):
    """forward (injected masks) and backward of the default single pass: (activations, gradients)."""
    triples = c["triples"] if triples is None else triples
    own = eng is None
    if own:
        eng = native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=0.8, norm_mode=norm,
                            max_edges=len(triples) if max_edges is None else max_edges)
    try:
        if own:
            eng.set_params(c["params"])
        eng.set_graph(triples)
        eng.forward(train=train, masks=c["masks"] if train else None)
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        grads = None
        if backward:
            eng.backward(c["dcodes"])
            grads = eng.get_grads()
        return acts, grads
    finally:
        if own:
            eng.close()


_RUNS = {}


def run_of(native, name, norm="intended"):
    """The engine's step on a case in a context of the case's own max_edges, once per module."""
    if (name, norm) not in _RUNS:
        c = case_of(name)
        _RUNS[(name, norm)] = step(native, c, norm=norm, max_edges=c["max_edges"])
    return _RUNS[(name, norm)]


def check_forward(name, acts, acts64):
    report = []
    for l, (a, b) in enumerate(zip(acts, acts64)):
        assert np.isfinite(a).all(), "%s H%d non-finite" % (name, l)
        worst, l2 = helpers.error_against(b, a)
        report.append("H%d %.1e/%.1e" % (l, worst, l2))
        assert worst <= FWD_MAX and l2 <= FWD_L2, "%s H%d against float64: max %.2e l2 %.2e" % (name, l, worst, l2)
    return report


def check_against_float64(name, acts, grads, norm="intended"):
    """test_float64_tie_break's procedure and bars."""
    c = case_of(name)
    report = check_forward(name, acts, forward64(name, norm))
    g64 = helpers.float64_grads_at(c, acts, norm)
    g32 = oracle.encoder_backward(c["params"], c["triples"], c["V"], c["L"], c["kind"], acts, c["dcodes"],
                                  mode="train", keep_prob=0.8, dropout_masks=c["masks"], norm_mode=norm)
    bad = []
    for k in sorted(g64):
        if k == "W_relation" or not np.abs(g64[k]).max() > 0:     # biases of the GCN layers: unconnected
            continue
        worst, l2 = helpers.error_against(g64[k], grads[k])
        oworst, ol2 = helpers.error_against(g64[k], g32[k])
        report.append("%s %.1e/%.1e (oracle %.1e/%.1e)" % (k, worst, l2, oworst, ol2))
        if not (worst <= GRAD_MAX and l2 <= GRAD_L2):
            bad.append("%s grad %s against float64: max %.2e l2 %.2e" % (name, k, worst, l2))
        if not l2 <= 4 * ol2 + 1e-7:
            bad.append("%s grad %s: l2 %.2e, the fp32 oracle's %.2e" % (name, k, l2, ol2))
    print(name, norm, "; ".join(report))
    assert not bad, bad


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("name,norm", [(n, "intended") for n in gg.FLOAT64_CASES] + [("giant_sd5_nb4", "tf_as_executed")])
def test_giant_rows_against_float64(native, name, norm):
    """The single pass in train mode with injected masks, then backward, on every case of the table but d = 1028 (the
    switch cases and the column-sum fallback among them)."""
    acts, grads = run_of(native, name, norm)
    check_against_float64(name, acts, grads, norm)


def test_evaluation_pass_against_float64(native):
    """train = False, forward only: what a full-graph evaluation runs."""
    name = "giant_sd5_nb4"
    acts, _ = step(native, case_of(name), train=False, backward=False)
    print(name, "test mode", "; ".join(check_forward(name, acts, forward64(name, mode="test"))))


# ------------------------------------------------------------------ 2. the test would notice a lost piece
def lost_piece_reference(c):
    """float64 forward on the graph whose LAST slot of row LOST_PIECE_ROW belongs to another vertex.  k_keys orders a row's
    slots by directed relation (r for an arriving edge, R + r for a leaving one), ties by incidence index: the last slot
    is the leaving edge of the largest relation, and of those the one with the largest index.  In the 2049-slot row it is
    the whole second piece."""
    t = np.array(c["triples"])
    out = np.flatnonzero(t[:, 0] == LOST_PIECE_ROW)
    e = int(out[t[out, 1] == t[out, 1].max()][-1])
    t[e, 0] = LOST_PIECE_TO
    with helpers.oracle_float64():
        p64 = {k: np.asarray(v, dtype=np.float64) for k, v in c["params"].items()}
        return oracle.encoder_forward(p64, t, c["V"], c["L"], c["kind"], mode="train", keep_prob=0.8,
                                      dropout_masks=c["masks"], norm_mode="intended")


def test_a_lost_piece_would_miss_the_bar(native):
    """The forward bar is tight enough to see ONE slot of a 2049-slot row go missing: against the float64 forward of the
    graph without that slot (the reference is perturbed, the kernel never runs on bad input) row 3 of H1 sits at seven
    times the bar: 1.45e-4 of scale between the two float64 references (the slot's own message is 3.1e-4 of scale, the
    last slots of the 4097- and 6000-slot rows 1.2e-4)."""
    c = case_of(LOST_PIECE_CASE)
    assert c["hubs"][LOST_PIECE_ROW] == gg.GIANT_ROW + 1
    acts, _ = run_of(native, LOST_PIECE_CASE)
    good, lost = forward64(LOST_PIECE_CASE)[1], lost_piece_reference(c)[1]
    scale = float(np.abs(lost).max())
    between = float(np.abs(good[LOST_PIECE_ROW] - lost[LOST_PIECE_ROW]).max()) / scale
    err = float(np.abs(acts[1][LOST_PIECE_ROW] - lost[LOST_PIECE_ROW]).max()) / scale
    ok = float(np.abs(acts[1][LOST_PIECE_ROW] - good[LOST_PIECE_ROW]).max()) / float(np.abs(good).max())
    print("lost piece: references %.2e apart, engine %.2e from the perturbed one, %.2e from the true one" % (between, err, ok))
    assert between > 4 * FWD_MAX
    assert err > FWD_MAX, "row %d of H1 is within the bar of a reference that lacks its last slot: %.2e" % (LOST_PIECE_ROW, err)
    assert ok <= FWD_MAX


# ------------------------------------------------------------------ 3. both forms, bitwise
@pytest.mark.parametrize("name", sorted(gg.GIANT_CASES))
@pytest.mark.parametrize("gen_dropout", [False, True])
def test_single_pass_equals_the_two_kernel_form_on_giant_rows(native, name, gen_dropout):
    """k_block_rows' pieces against k_combine's (the piece lists, the slab and the finish kernel are common to both):
    activations and gradients bitwise, b_emb within 2e-6 of scale -- every case, d = 1028 (float4 columns on the finish
    loop's second trip) included."""
    c = gg.GIANT_CASES[name]
    params, triples, masks, dcodes = (case_of(name)[k] for k in ("params", "triples", "masks", "dcodes")) \
        if c["float64"] else gg.giant_inputs(c)
    _single_pass_equals_two_kernel_form(native, c["V"], c["R"], c["d"], c["nb"], params, triples, masks, dcodes, gen_dropout)


# ------------------------------------------------------------------ 4. the switch
def switch_untouched(on, off_triples, dropped):
    """What the dropped edge (s, r, o) cannot reach.  H1: every row but s and o (their sums lose a message, their 1 / degree
    changes).  H2: every row outside T2 = {s, o} and their neighbours.  Gradients of the top layer's relation weights:
    dL/dW_f2[q] and dL/dW_b2[q] sum n_m D2[dst_m] x H1[src_m] over the messages m of relation q with D2 = dcodes (no
    gate above the top layer), so they are untouched for every relation q without an edge at s or o.  Everything else
    -- dL/dW_self (sums over all rows), the bottom layer's gradients and dL/dW_emb (through relu'(H1) on T2, which
    holds hub rows: every vertex of this graph is within two hops of the edge) -- depends on it."""
    s, _, o = (int(x) for x in dropped)
    t = off_triples
    t1 = np.zeros(on["V"], dtype=bool)
    t1[[s, o]] = True
    t2 = t1.copy()
    t2[t[t1[t[:, 2]], 0]] = True
    t2[t[t1[t[:, 0]], 2]] = True
    rel = np.ones(on["R"], dtype=bool)
    rel[on["triples"][t1[on["triples"][:, 0]] | t1[on["triples"][:, 2]], 1]] = False
    return ~t1, ~t2, rel


def test_both_sides_of_the_switch_agree(native):
    """2E = 65,538 sums the rows of 2049 .. 6000 slots piece by piece, 2E = 65,536 as ordinary long rows (and halves the
    relation chunk): each side passes the float64 bars (test_giant_rows_against_float64), and where the one edge between
    them cannot reach the two engines agree within twice the bars -- both are within one bar of the same float64
    values there.  The summation order differs, so bitwise equality is not expected."""
    on, off = case_of("giant_switch_on"), case_of("giant_switch_off")
    (a_on, g_on), (a_off, g_off) = run_of(native, "giant_switch_on"), run_of(native, "giant_switch_off")
    k = gg.free_edge(on)
    rows1, rows2, rel = switch_untouched(on, off["triples"], on["triples"][k])
    nh = len(on["hubs"])
    assert rows1.sum() == on["V"] - 2 and rows1[:nh].all() and rel.sum() >= on["R"] // 2
    report = []
    np.testing.assert_array_equal(a_on[0], a_off[0])
    for tag, x, y, keep, bar_max, bar_l2 in (
            [("H1", a_on[1], a_off[1], rows1, FWD_MAX, FWD_L2), ("H2", a_on[2], a_off[2], rows2, FWD_MAX, FWD_L2)] +
            [(w, g_on[w], g_off[w], rel, GRAD_MAX, GRAD_L2) for w in ("W_f2", "W_b2")]):
        assert keep.any(), tag
        scale = float(np.abs(y).max())
        xs, ys = x[keep].astype(np.float64), y[keep].astype(np.float64)
        worst = float(np.abs(xs - ys).max()) / scale
        l2 = float(np.sqrt(((xs - ys) ** 2).sum() / (ys ** 2).sum()))
        report.append("%s %.1e/%.1e over %d" % (tag, worst, l2, int(keep.sum())))
        assert worst <= 2 * bar_max and l2 <= 2 * bar_l2, "%s across the switch: max %.2e l2 %.2e" % (tag, worst, l2)
    print("switch:", "; ".join(report))


# ------------------------------------------------------------------ 5. column-sum fallback
def test_column_sum_fallback_gives_the_same_gradients(native):
    """A context sized for 1,200,000 edges cannot keep giant_cap = 1172 part rows beside the row kernel's own: block_rows()
    leaves the bias gradient to the separate column-sum pass.  Against a context of the graph's own size (partials from
    the row kernel and k_colsum_giant_rows): everything bitwise but b_emb, the same terms in another order."""
    name = "giant_colsum_fallback"
    c = case_of(name)
    assert not gg.colsum_in_kernel(c["V"], c["d"], c["E"], c["max_edges"], c["nb"])
    assert gg.colsum_in_kernel(c["V"], c["d"], c["E"], c["E"], c["nb"])
    (fa, fg), (ia, ig) = run_of(native, name), step(native, c, max_edges=c["E"])
    for l in range(c["L"] + 1):
        np.testing.assert_array_equal(fa[l], ia[l], err_msg="H%d" % l)
    scale = np.abs(ig["W_emb"]).astype(np.float64).sum(axis=0).max()
    for k in fg:
        if k == "b_emb":
            assert np.abs(fg[k].astype(np.float64) - ig[k]).max() <= 2e-6 * scale
            want = ig["W_emb"].astype(np.float64).sum(axis=0)
            assert np.abs(fg[k] - want).max() <= 2e-6 * scale and np.abs(ig[k] - want).max() <= 2e-6 * scale
            continue
        np.testing.assert_array_equal(fg[k], ig[k], err_msg=k)


# ------------------------------------------------------------------ 6. one context, three graphs
def small_graph(c):
    """kernel_grid's 3,000-edge graph (rows of 33, 100 and 400 slots) at the case's V and R: the cut is off."""
    return kg.grid_triples(dict(V=c["V"], R=c["R"], E=kg.E_GRID, hubs=(33, 100, 400), seed=c["seed"] + 1))


def assert_same_step(got, want, tag):
    for l, (x, y) in enumerate(zip(got[0], want[0])):
        np.testing.assert_array_equal(x, y, err_msg="%s H%d" % (tag, l))
    for k in want[1]:
        np.testing.assert_array_equal(got[1][k], want[1][k], err_msg="%s %s" % (tag, k))


def test_one_context_alternates_between_cut_and_uncut_graphs(native):
    """What train.py does between training steps and evaluation: a minibatch graph (cut off), the full graph (cut on: the
    piece slab is allocated at this point, the counters re-zeroed by k_keys), the minibatch graph again (the rows of the
    giant list are ordinary rows once more).  Every step bitwise that of a fresh engine given only its graph."""
    c = case_of("giant_sd5_nb4")
    small = small_graph(c)
    assert not gg.giant_on(len(small)) and gg.giant_on(c["E"])
    fresh = [step(native, c, triples=t, max_edges=c["E"]) for t in (small, c["triples"])]
    with native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        for i, (t, want) in enumerate(((small, fresh[0]), (c["triples"], fresh[1]), (small, fresh[0]))):
            assert_same_step(step(native, c, triples=t, eng=eng), want, "graph %d" % i)
    assert_same_step(fresh[1], run_of(native, "giant_sd5_nb4"), "fresh")


def device_steps(native, c, graphs, prefetch_at=None):
    """rgcn_step_device on each graph in turn (generated dropout, seed 40 + i); prefetch_at: that graph is prepared
    beside the step before it through rgcn_prefetch_graph_device."""
    out = []
    with native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        dc = eng.to_device(c["dcodes"])
        bufs = [eng.to_device(np.ascontiguousarray(t)) for _, t in graphs]
        try:
            for i, (seed, t) in enumerate(graphs):
                eng.step_device(bufs[i], len(t), dc, train=True, seed=seed)
                if prefetch_at is not None and i + 1 == prefetch_at:
                    eng.prefetch_graph_device(bufs[i + 1], len(graphs[i + 1][1]))
                out.append(([eng.activation(l) for l in range(c["L"] + 1)], eng.get_grads()))
        finally:
            for b in bufs + [dc]:
                b.free()
    return out


def test_prefetched_cut_graph_between_uncut_ones(native):
    """The same alternation with the full graph prepared on the prefetch stream into the second graph set
    (rgcn_prefetch_graph_device, as test_gpu_parity.py::test_prefetched_graph_gives_identical_step) and adopted by
    rgcn_step_device: bitwise the steps of fresh engines."""
    c = case_of("giant_sd5_nb4")
    small = small_graph(c)
    graphs = [(40, small), (41, c["triples"]), (42, small)]
    got = device_steps(native, c, graphs, prefetch_at=1)
    for i, g in enumerate(graphs):
        assert_same_step(got[i], device_steps(native, c, [g])[0], "graph %d" % i)


# ------------------------------------------------------------------ 7. determinism with many giant rows
def test_many_giant_rows_are_deterministic(native):
    """66 giant rows: piece ids and the giant-row list come from atomic counters, the finish kernel takes a second trip,
    k_colsum_giant_rows ranks 66 part rows by vertex id -- two fresh engines give bit-identical results, and db_emb is the
    float64 column sum of dW_emb to 2e-6 of scale."""
    name = "giant_many"
    c = case_of(name)
    first, second = run_of(native, name), step(native, c)
    assert_same_step(second, first, name)
    grads = first[1]
    want = grads["W_emb"].astype(np.float64).sum(axis=0)
    scale = np.abs(grads["W_emb"]).astype(np.float64).sum(axis=0).max()
    assert np.abs(grads["b_emb"] - want).max() <= 2e-6 * scale
