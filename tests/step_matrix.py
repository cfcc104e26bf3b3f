"""The decoder's loss terms and row weights on every encoder form: the table of cases and the composed float64 mirror.

Six decoder-side options of the fused train steps -- the relation-softmax term, the entity-softmax term, self-adversarial
row weights, relation corruptions, type-constrained negatives, reciprocal relations -- each have a GPU test of their own,
all on ("block", 4) and ("basis", 2) at V 80, d 20, code_dim == dim.  Six encoder forms -- highway, the output transform,
basis_tdiag, basis_pdiag, the one-hot first layer, local norms -- change what train_step_tail (csrc/rgcn_api.hip) and
bwd_begin (csrc/rgcn_schedule.hip) do with dL/dcodes, and no test put an option on one of them.  STEP_MATRIX is that
product; tests/test_step_matrix.py keeps it honest without a GPU, tests/test_gpu_step_matrix.py runs it.

Nothing here restates an operation: compose() adds the mirrors of tests/relation_softmax_reference.py,
tests/entity_softmax_reference.py and tests/adversarial_reference.py on one batch, and forward64() / encoder_grads() run a
form's own float64 forward and reverse mode (helpers.float64_grads_at, times_diag_reference, add_diagonal_reference,
featureless_reference, and fullgraph_grid's chain of highway_reference, local_norm_reference and
output_transform_reference).

Every form: L 2, keep 0.8, R 8 (2 R <= V: reciprocal relations are legal), local_norm_reference.extended_graph at 300
edges (vertex V - 1 is a hub of 48 slots, past kLongRow = 32; relation R - 1 has no edge).  `tdiag` takes the
narrowest row of tests/tdiag_grid.py, d 9 with B 8, and `pdiag` the row of the same shape of tests/pdiag_grid.py (d 9 is
also a scalar code width).
"""
import numpy as np

import add_diagonal_reference as adr
import adversarial_reference as adv
import entity_softmax_reference as esr
import featureless_reference as flr
import fullgraph_grid as fg
import helpers
import highway_reference as hr
import local_norm_reference as lnr
import reciprocal_reference as rr
import relation_softmax_reference as rsr
import times_diag_reference as tdr

KEEP, REG, L, R, E = 0.8, 0.01, 2, 8, 300
ALPHA, RELSM_WEIGHT, ENTSM_WEIGHT = adv.ALPHA, 0.6, 0.5
FWD_ATOL = fg.FWD_ATOL
ENERGY_STD = 1.5
P_STEP, K_STEP = 65, 3          # the X/Y steps: 65 positives (2 P = 130 rows of the entity term: past one 128-row tile), 3 negatives each
N_BATCH, RATE, KEEP_EDGES, M_REL, LEADING = 200, 2, 120, 2, 77      # the minibatch steps


# ----------------------------------------------------------------------------- encoder forms
def _form(name, seed, kind="block", nb=4, d=20, V=80, input_mode="embedding", skip="none", norm="intended", code_dim=0):
    return dict(name=name, seed=seed, kind=kind, nb=nb, d=d, V=V, R=R, L=L, input_mode=input_mode, skip=skip, norm=norm,
                code_dim=code_dim, dc=code_dim or d)


FORM_LIST = [
    _form("block", 9101),
    _form("basis", 9102, kind="basis", nb=2),
    _form("tdiag", 9103, kind="basis_tdiag", nb=8, d=9),
    _form("pdiag", 9104, kind="basis_pdiag", nb=8, d=9),
    _form("onehot", 9105, kind="basis", nb=2, input_mode="onehot"),
    _form("highway", 9106, skip="highway"),
    _form("out8", 9107, code_dim=8, V=83),                       # V % 4 = 3: the entity term's nn_padded route
    _form("out6", 9108, kind="basis", nb=2, code_dim=6, V=83),   # dc % 4 != 0: the scalar paths of both terms and of the weights
    _form("local", 9109, norm="local"),
    _form("all", 9110, skip="highway", norm="local", code_dim=8, V=83),
]
FORMS = {f["name"]: f for f in FORM_LIST}
MASKED_FORMS = ("block", "out8", "out6")
MINIBATCH_FORMS = ("block", "out8", "highway")
OFF_FORMS = ("out8", "highway")


def family(f):
    """whose float64 forward and reverse mode the form takes"""
    if f["kind"] == "basis_tdiag":
        return "tdiag"
    if f["kind"] == "basis_pdiag":
        return "pdiag"
    if f["input_mode"] == "onehot":
        return "onehot"
    if f["skip"] == "none" and f["norm"] == "intended" and not f["code_dim"]:
        return "plain"
    return "chain"


def readable(f):
    """whether every activation the reverse mode needs can be read back behind a fused step (a highway context keeps
    N_l and T_l of the layer run last only)"""
    return f["skip"] != "highway"


def unused_bias(f, name):
    """b<l> of a block or basis layer: created and never added; its gradient is all zeros"""
    return f["kind"] in ("block", "basis") and fg.unused_bias(name)


def weight_names(f):
    """rgcn_param_info names of the form's context"""
    fam = family(f)
    if fam == "tdiag":
        return tdr.weight_names(L)
    if fam == "pdiag":
        return adr.weight_names(L)
    if fam == "onehot":
        return flr.weight_names(L)
    return fg.weight_names(f)


# ----------------------------------------------------------------------------- decoder options
MODES = {   # sampling mode -> (entity sampler of reciprocal_reference.sampler_rows, relation rows, reciprocal tail)
    "plain": ("plain", 0, False), "exclusive": ("exclusive", 0, False), "relation": ("plain", M_REL, False),
    "typed": ("typed", 0, False), "typed+relation": ("typed", M_REL, False), "reciprocal": ("plain", 0, True),
    "typed+reciprocal": ("typed", 0, True),
}


def _row(form, step, mode=None, entsm=ENTSM_WEIGHT, count=0, masked=False, off=False):
    name = "%s-%s" % (form, "all-terms" if step == "xy" and not masked else "masked" if step == "xy" else mode)
    if off:
        name = "%s-off" % form
    return dict(name=name, form=form, step=step, mode=mode, adv=ALPHA, relsm=RELSM_WEIGHT, entsm=entsm, entsm_count=count,
                relsm_exclusive=masked, entsm_exclusive=masked and entsm > 0, off=off)


def _minibatch_rows(form):
    rows = []
    for mode in MODES:
        recip = MODES[mode][2]
        rows.append(_row(form, "minibatch", mode, entsm=0.0 if recip else ENTSM_WEIGHT,       # the entity term is refused
                         count=LEADING if mode == "plain" else 0, masked=mode == "exclusive"))  # under reciprocal relations
    return rows


STEP_MATRIX = ([_row(f["name"], "xy") for f in FORM_LIST] + [_row(f, "xy", masked=True) for f in MASKED_FORMS]
               + [r for f in MINIBATCH_FORMS for r in _minibatch_rows(f)] + [_row(f, "off", off=True) for f in OFF_FORMS])
CASES = {c["name"]: c for c in STEP_MATRIX}
ALL_TERMS = [c["name"] for c in STEP_MATRIX if c["step"] == "xy" and not c["relsm_exclusive"]]
MASKED = [c["name"] for c in STEP_MATRIX if c["step"] == "xy" and c["relsm_exclusive"]]
MINIBATCH = [c["name"] for c in STEP_MATRIX if c["step"] == "minibatch"]
OFF = [c["name"] for c in STEP_MATRIX if c["off"]]
# the three cases whose composed gradient tests/test_step_matrix.py holds to central differences
GRADIENT_CASES = ("block-all-terms", "out6-masked", "block-typed+reciprocal")


# ----------------------------------------------------------------------------- inputs
def extra_known(triples, V):
    """Known triples beside the graph's, so that the masks matter: of the graph's distinct triples, in order, two of every
    three get another relation on their pair (the relation term's mask); the even ones one to three more objects of
    (s, r), the odd ones more subjects of (r, o) (the entity term's mask, as test_gpu_entity_softmax.masked_case's)."""
    t = np.unique(np.asarray(triples).reshape(-1, 3), axis=0)
    rng = np.random.RandomState(len(t) + V)
    out = []
    for n, (s, r, o) in enumerate(t.tolist()):
        if n % 3:
            out.append((s, (r + 1 + n % 2) % R, o))
        for e in rng.choice(V, size=1 + n % 3, replace=False).tolist():
            out.append((s, r, e) if n % 2 == 0 else (e, r, o))
    return np.asarray(out, dtype=np.int32)


def form_inputs(f):
    """The form with its graph, weights (W_relation [V, dc]), seeded masks and what the decoder batches are drawn from:
    `known` (the graph and extra_known), `batch` (the first N_BATCH distinct triples, a minibatch step's positives), and
    the X/Y step's batch -- P_STEP positives from the graph, then K_STEP entity corruptions of each, group by group."""
    c = dict(f)
    V, d, kind, nb, seed = f["V"], f["d"], f["kind"], f["nb"], f["seed"]
    graph = lnr.extended_graph(V, R, E, seed=seed)
    fam = family(f)
    if fam == "tdiag":
        m = tdr.make_case(V, R, d, L, nb, graph, seed=seed, keep=KEEP)
    elif fam == "pdiag":
        m = adr.make_case(V, R, d, L, nb, graph, seed=seed, keep=KEEP)
    elif f["skip"] == "highway":
        m = hr.make_case(V, R, d, L, kind, nb, graph, seed=seed, keep=KEEP)
    else:
        rng = np.random.RandomState(seed)
        if fam == "onehot":
            params = flr.init_params(V, R, d, L, nb, rng)
        else:
            params = helpers.make_case(V, R, d, L, kind, nb, 0, seed=seed, keep=KEEP)[0]
        m = {"params": params, "masks": [(rng.rand(V, d) < KEEP).astype(np.uint8) for _ in range(L)]}
    c["params"], c["masks"] = dict(m["params"]), m["masks"]
    rng = np.random.RandomState(seed + 5)
    if f["code_dim"]:
        from relationprediction_amd.common.shared_functions import glorot_variance
        cd = f["code_dim"]
        c["params"]["W_out"] = rng.normal(0, glorot_variance([d, cd]), size=(d, cd)).astype(np.float32)
        c["params"]["b_out"] = (rng.randn(cd) * 0.3).astype(np.float32)
        c["params"]["W_relation"] = rng.randn(V, cd).astype(np.float32)
    assert c["params"]["W_relation"].shape == (V, f["dc"]) and sorted(c["params"]) == sorted(weight_names(f))
    c["triples"] = graph
    c["known"] = np.concatenate([graph, extra_known(graph, V)]).astype(np.int32)
    c["batch"] = np.unique(graph, axis=0)[:N_BATCH].astype(np.int32)
    assert len(c["batch"]) == N_BATCH
    rng = np.random.RandomState(seed + 6)
    pos = graph[rng.choice(len(graph), P_STEP, replace=False)].astype(np.int32)
    rows = [pos]
    for _ in range(K_STEP):
        neg = pos.copy()
        neg[np.arange(P_STEP), rng.randint(0, 2, P_STEP) * 2] = rng.randint(0, V, P_STEP)
        rows.append(neg)
    c["X"] = np.concatenate(rows).astype(np.int32)
    c["Y"] = np.concatenate([np.ones(P_STEP), np.zeros(P_STEP * K_STEP)]).astype(np.float32)
    c["keep"] = KEEP
    # The initialisers leave codes of 5 to 40 in magnitude and energies in the hundreds, at which every softmax of the
    # options is one-hot: its gradient vanishes and a wrong one would pass.  Every energy of the decoder and of both terms is
    # linear in W_relation, so W_relation is scaled until the X/Y batch's energies (at the float64 forward under the seeded
    # masks) have standard deviation ENERGY_STD.
    x, _ = adv.float64_energies(forward64(c, c["masks"], graph)["codes"], c["params"]["W_relation"], c["X"])
    c["params"]["W_relation"] = (c["params"]["W_relation"] * np.float32(ENERGY_STD / x.std())).astype(np.float32)
    return c


def case_inputs(name):
    """a row of STEP_MATRIX with its form's inputs: what compose() and encoder_grads() take as `case`"""
    row = CASES[name]
    return dict(form_inputs(FORMS[row["form"]]), **row)


def mirror_batch(case, seed):
    """(X, Y, n_pos) of a case: the X/Y step's own batch, or what the minibatch step's samplers write under the case's mode
    for negative seed `seed` (reciprocal_reference over the samplers' own mirrors)"""
    c = case
    if case["step"] != "minibatch":
        return c["X"], c["Y"], P_STEP
    kind, m, recip = MODES[case["mode"]]
    X, Y = rr.sampler_rows(kind, c["batch"], c["known"], RATE, m, c["V"], R, seed)
    if recip:
        X, Y = rr.transform(c["batch"], X, Y, RATE, m, R, seed)
    return X, Y, N_BATCH


# ----------------------------------------------------------------------------- the composed mirror of the decoder side
def compose(case, codes, X, Y, n_pos, w_relation=None, exact_query=False, row_weights=None):
    """float64 loss, dcodes [V, dc] and dW_relation [rows of W_relation, dc] of the decoder plus every enabled term of
    `case` at the given codes, as train_step_tail adds them:

      the decoder over all N rows; under `adv` weighted by adversarial_reference's weights of the groups (row i >= n_pos
      is a negative of positive i mod n_pos).  Under a reciprocal mode the batch ends in n_pos inverse positives
      (s, R + r, o), which stand outside the groups with weight 1 (optimizer_fill behind adversarial_weights) and read
      row R + r of W_relation like any other row (reciprocal_reference);
      `relsm`: relation_softmax_reference.term over the leading n_pos rows.  relation_softmax_compute runs its softmax
      over c->R relations -- the first R rows of W_relation -- under every mode, reciprocal included: the rows R + r take
      no part in it, and the term adds to rows [0, R) of dW_relation only;
      `entsm`: entity_softmax_reference.term over the leading min(entsm_count, n_pos) rows (all n_pos where the count is
      0), over all V entities, adding to rows [0, R) of dW_relation (its rows' relations are the positives').
      Under `relsm_exclusive` / `entsm_exclusive` the term's candidates are masked by the case's `known`.
    case: case_inputs' dict; w_relation: another W_relation than the case's (a finite-difference check moves it).

    exact_query: the terms' query rows in float64 from the start; row_weights [N]: the decoder's weights given (they are
    constants of the gradient) -- what a finite-difference check of the composed loss needs.
    Returns a dict: loss, dcodes, dW, w and tol (the adversarial weights and their tolerance; None without `adv`), and the
    parts `decoder`, `plain` (the unit-weight decoder's loss), `rel`, `ent` (the terms' own dicts, or None)."""
    W = case["params"]["W_relation"] if w_relation is None else w_relation
    known = case["known"]
    N = len(X)
    tail = n_pos if case["mode"] and MODES[case["mode"]][2] else 0
    if tail:
        assert np.array_equal(X[N - tail:, 1], rr.shift_relation(X[:n_pos, 1], R)) and (np.asarray(Y[N - tail:]) == 1).all()
    out = {"w": None, "tol": None, "rel": None, "ent": None}
    out["plain"] = rsr.decoder(codes, W, X, Y, REG)[0]
    if case["adv"]:
        if row_weights is not None:
            w, tol = np.asarray(row_weights, dtype=np.float64), None
        elif tail:
            head = adv.weights(codes, W, X[:N - tail], n_pos, case["adv"])
            w, tol = np.concatenate([head["w"], np.ones(tail)]), np.concatenate([head["tol"], np.zeros(tail)])
        else:
            head = adv.adversarial_decoder(codes, W, X, Y, n_pos, case["adv"], REG)
            w, tol = head["w"], head["tol"]
        dec = adv.weighted_decoder(codes, W, X, Y, w, REG)
        loss, dcodes, dW = dec["loss"], np.array(dec["dcodes"]), np.array(dec["dW"])
        out["w"], out["tol"] = w, tol
    else:
        loss, dcodes, dW = rsr.decoder(codes, W, X, Y, REG)
    out["decoder"] = loss
    if case["relsm"]:
        t = rsr.term(codes, W, X[:n_pos], R, case["relsm"], known=known if case["relsm_exclusive"] else None,
                     exact_query=exact_query)
        loss, dcodes = loss + t["loss"], dcodes + t["dcodes"]
        dW[:R] += t["dW"]
        out["rel"] = t
    if case["entsm"]:
        assert not tail, "the entity term is refused under reciprocal relations"
        n_ent = min(case["entsm_count"], n_pos) if case["entsm_count"] else n_pos
        t = esr.term(codes, W, X[:n_ent], case["entsm"], known=known if case["entsm_exclusive"] else None,
                     exact_query=exact_query)
        assert not t["dW"][R:].any()
        loss, dcodes, dW = loss + t["loss"], dcodes + t["dcodes"], dW + t["dW"]
        out["ent"] = t
    out["loss"], out["dcodes"], out["dW"] = float(loss), dcodes, dW
    return out


# ----------------------------------------------------------------------------- the encoder side
def _chain_case(c, masks, graph, dcodes=None):
    cc = dict(c, masks=masks, triples=graph)
    if dcodes is not None:
        cc["dcodes"] = np.asarray(dcodes, dtype=np.float64)
    return cc


def forward64(c, masks, graph):
    """The form's own float64 forward in train mode with the given dropout masks: {"H": [H0 (None on a one-hot form),
    H1 .. HL], "N" / "T" (highway forms), "codes": [V, dc]}"""
    fam, V, p = family(c), c["V"], c["params"]
    if fam == "tdiag":
        acts = {"H": tdr.forward(p, graph, V, L, keep=KEEP, masks=masks, norm=c["norm"])[0]}
    elif fam == "pdiag":
        acts = {"H": adr.forward(p, graph, V, L, keep=KEEP, masks=masks, norm=c["norm"])[0]}
    elif fam == "onehot":
        acts = {"H": flr.forward(p, graph, V, L, keep=KEEP, masks=masks)}
    elif fam == "plain":
        acts = {"H": [np.asarray(a) for a in helpers.float64_forward(_chain_case(c, masks, graph), keep=KEEP)]}
    else:
        acts = fg.reference_forward(_chain_case(c, masks, graph), masks=masks, triples=graph)
    acts.setdefault("codes", acts["H"][L])
    return acts


def encoder_grads(c, masks, graph, dcodes64, acts=None):
    """float64 gradient of every encoder parameter (W_relation is the decoder side's) under dL/dcodes = dcodes64: the
    form's own reverse mode at `acts` -- an engine's own activations ({"H": [..]}: its own relu gates) -- or, acts None,
    at the form's float64 forward with the engine's dropout masks."""
    fam, V, p = family(c), c["V"], c["params"]
    if acts is None:
        acts = forward64(c, masks, graph)
    top = np.asarray(dcodes64, dtype=np.float64)
    stack = {k: v for k, v in p.items() if k != "W_relation"}
    if fam == "tdiag":
        return tdr.backward(stack, graph, V, L, acts["H"], top, keep=KEEP, masks=masks, norm=c["norm"])
    if fam == "pdiag":
        return adr.backward(stack, graph, V, L, acts["H"], top, keep=KEEP, masks=masks, norm=c["norm"])
    if fam == "onehot":
        return flr.backward(stack, graph, V, L, acts["H"], top, keep=KEEP, masks=masks)
    if fam == "plain":
        g = helpers.float64_grads_at(_chain_case(c, masks, graph, top), acts["H"], keep=KEEP)
        return {k: np.asarray(v) for k, v in g.items() if k != "W_relation"}
    return fg.reference_backward(_chain_case(c, masks, graph, top), acts, masks=masks, triples=graph)


def mirror_step(case, X, Y, n_pos, masks, graph, acts=None):
    """The whole step in float64: compose() at the codes of `acts` -- an engine's own {"H": [..], "codes": ..}; None: the
    form's float64 forward with the engine's masks -- pushed through encoder_grads at the same activations.
    Returns (composed dict, {name: gradient}, W_relation's among them)."""
    if acts is None:
        acts = forward64(case, masks, graph)
    out = compose(case, acts["codes"], X, Y, n_pos)
    g = dict(encoder_grads(case, masks, graph, out["dcodes"], acts=acts))
    g["W_relation"] = out["dW"]
    assert set(g) == set(weight_names(case)), sorted(set(g) ^ set(weight_names(case)))
    return out, g


# ----------------------------------------------------------------------------- the checks both test files share
def check_options_count(case, out, n_pos):
    """each enabled option matters on this case's batch: what a GPU comparison rests on (conditions, not tolerances)"""
    name = case["name"]
    if case["adv"]:
        neg = out["w"][n_pos:len(out["w"]) - (n_pos if MODES.get(case["mode"], (0, 0, False))[2] else 0)]
        assert neg.max() >= 1.5 and neg.min() <= 0.5, (name, neg.min(), neg.max())
        assert abs(out["decoder"] - out["plain"]) > 1e-3, name
    for key, on in (("rel", case["relsm"]), ("ent", case["entsm"])):
        if on:
            assert abs(out[key]["loss"]) > 1e-3, (name, key)
            if case[{"rel": "relsm_exclusive", "ent": "entsm_exclusive"}[key]]:
                masked_rows = int((~out[key]["mask"]).any(axis=1).sum())
                assert 3 * masked_rows >= len(out[key]["mask"]), (name, key, masked_rows)
    assert np.abs(out["dcodes"]).max() > 0 and np.abs(out["dW"]).max() > 0


def check_gradients(case, grads, g64, rel=1e-3, tag=""):
    """The fused-step tests' bar: helpers.assert_close(rel = 1e-3) of every parameter's gradient against the mirror; no
    tensor all zeros but the layers' unused biases, which are zero on both sides.  rel: the bar of the encoder's own
    parameters where the form's own test has a tighter one (helpers.assert_close's default 2e-4 at an engine's own
    activations: fullgraph_grid.check_gradients); W_relation keeps 1e-3.  Returns the report entries
    `name max / l2 relative error`."""
    c = case
    report = []
    for n in weight_names(c):
        worst, l2 = helpers.error_against(g64[n], grads[n])
        report.append("%s %.1e/%.1e" % (n, worst, l2))
        if unused_bias(c, n):
            assert not np.asarray(grads[n]).any() and not np.asarray(g64[n]).any(), n
            continue
        assert np.abs(g64[n]).max() > 0 and np.abs(grads[n]).max() > 0, "%s%s %s is all zeros" % (tag, case["name"], n)
        helpers.assert_close(grads[n], g64[n], rel=1e-3 if n == "W_relation" else rel, name="%s%s %s" % (tag, case["name"], n))
    return report
