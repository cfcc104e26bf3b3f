"""The compiled variants of the DistMult decoder's kernels and the cases that reach every one of them.

decoder_compute (relationprediction_amd/csrc/decoder.hip) picks, from d, R and the batch:
  energies   k_dec_energy_rel<VEC, T> (one relation chunk per workgroup, relation-gradient partials fused in) while a
             row fits T <= 4 register tiles of 64 lanes, else k_dec_energy<VEC> + k_dec_rel_partial<VEC>;
  entity     k_dec_entity_lines<RLDS> (d % 4 == 0: column bands of one cache line, 8 bands per pass, the relation band
             in LDS when R * 128 B <= 64 KB), else k_dec_entity_grad<1, TPR>; rows of more than kDecLongRow incidences
             in pieces of kDecPiece, added up by k_dec_long_finish<VEC>;
  relation   chunks of kDecChunk triples per relation, summed by k_dec_rel_reduce (4 chunks per turn + a tail);
  tiled      a batch the negative sampler wrote: only the first copies sorted by relation (k_dec_expand);
  weighted   row_weights != nullptr: the WEIGHTED instantiation of either energy kernel (a weight per row on its loss
             term and its dx).
The functions below mirror those formulas on the host, so that a test can state which cell a case reaches; DECODER_CASES
is one case per cell and per boundary of the formulas, each with a batch of exact incidence and relation counts;
WEIGHTED_CASES holds every energy cell under both orders, with case_weights' built weights.
tests/test_decoder_grid.py keeps the table honest without a GPU; tests/test_gpu_train_step.py and
tests/test_gpu_decoder_weighted_grid.py run it.
"""
import numpy as np

BLOCK_SIZES = (1, 2, 3, 4, 5, 8)      # block_msgs.hip:184-192: the block sizes d / nb the encoder is compiled for
MAX_BLOCKS = 512                      # config_check.h (check_config)
LONG_ROW = 256                        # decoder.hip:27 (kDecLongRow): a row with more incidences is cut into pieces
PIECE = 512                           # decoder.hip:28 (kDecPiece): incidences per piece
CHUNK = 128                           # decoder.hip:30 (kDecChunk): triples per relation chunk
LINE = 32                             # decoder.hip:426 (kLine): floats per (row, band) of the line form
BANDS_PER_PASS = 8                    # decoder.hip:523: workgroup x takes bands x, x + 8, ...
MAX_DECODER_TRIPLES = 1 << 29         # include/rgcn.h (RGCN_MAX_DECODER_TRIPLES)

ENERGY_CELLS = [("energy_rel", 4, 1), ("energy_rel", 4, 2), ("energy_rel", 4, 4),
                ("energy_rel", 1, 1), ("energy_rel", 1, 2), ("energy_rel", 1, 4),
                ("energy", 4, None), ("energy", 1, None)]
ENTITY_CELLS = [("lines", True), ("lines", False), ("rows", 1, 64), ("rows", 1, 128), ("rows", 1, 256)]


def vec_width(d):
    """decoder.hip:939: float4 columns when d % 4 == 0 (the engine's buffers are 16-byte aligned)."""
    return 4 if d % 4 == 0 else 1


def energy_cell(d):
    """decoder.hip:945-947: fused while nvec_e <= 256, T = 1 / 2 / 4 register tiles for up to 64 / 128 / 256 vectors."""
    vec = vec_width(d)
    nvec = d // vec
    if nvec > 256:
        return ("energy", vec, None)
    return ("energy_rel", vec, 1 if nvec <= 64 else (2 if nvec <= 128 else 4))


def rel_partial_passes(d):
    """decoder.hip:588: k_dec_rel_partial (unfused rows only) walks the row in passes of 128 column vectors."""
    return -(-(d // vec_width(d)) // 128)


def relation_lds(R):
    """decoder.hip:1016-1017: the line form keeps the relation band [R][32] floats in LDS up to 64 KB."""
    return R * LINE * 4 <= 64 * 1024


def entity_tpr(d):
    """decoder.hip:1029 (row_walk.h:48, row_lanes): lanes per row of k_dec_entity_grad."""
    nvec = d // vec_width(d)
    return 64 if nvec <= 64 else (128 if nvec <= 128 else 256)


def entity_cell(d, R):
    """decoder.hip:1003: the line form whenever the rows are float4-addressable, else the full-row kernel."""
    if vec_width(d) == 4:
        return ("lines", relation_lds(R))
    return ("rows", 1, entity_tpr(d))


def bands(d):
    """decoder.hip:840: column bands of one line; the last one partial when d % 32 != 0."""
    return -(-d // LINE)


def band_passes(d):
    """decoder.hip:523: passes of the line form's band loop (8 bands per pass, one per XCD)."""
    return -(-bands(d) // BANDS_PER_PASS)


def pieces(incidences):
    """decoder.hip:129-132: pieces of a long row (0 for a row the short-row kernels take)."""
    return -(-incidences // PIECE) if incidences > LONG_ROW else 0


def chunks(triples):
    """decoder.hip:98: chunks of one relation's triples."""
    return -(-triples // CHUNK)


def copies(case):
    """decoder.hip:884-888: a batch the sampler tiled is decoded as `rate + 1` copies when its period n is > 1."""
    if case.get("rate") is None or case["n"] <= 1:
        return 1
    return case["rate"] + 1


def cell_of(case):
    """The compiled variants a case reaches: (energy cell, entity-gradient cell)."""
    return energy_cell(case["d"]), entity_cell(case["d"], case["R"])


def incidences(X, V):
    """Incidences of every entity row over both sides (decoder.hip:42-55: 2N keys, a self edge counts twice)."""
    X = np.asarray(X).reshape(-1, 3)
    return np.bincount(np.concatenate([X[:, 0], X[:, 2]]), minlength=V)


# ----------------------------------------------------------------------------- the table
# Entity e < 7 has exactly ENTITY_COUNTS[e] incidences: no row, one, the longest short row, the first long row (one
# piece), one full piece, two pieces (the second of one incidence), three pieces.  Relation r < 7 has exactly
# REL_COUNTS[r] triples: none, one, a partial chunk, one short of a chunk, a chunk, one past it, five chunks (one turn of
# k_dec_rel_reduce's 4-way unroll + its tail).  A tiled batch holds TILED_REL_COUNTS[copies] of relation r among its n
# first copies, so that the decoded counts (x copies) sit on and just past the chunk boundaries.
ENTITY_COUNTS = (0, 1, 256, 257, 512, 513, 1025)
REL_COUNTS = (0, 1, 5, 127, 128, 129, 640)
TILED_REL_COUNTS = {11: (0, 1, 5, 12, 128, 129), 2: (0, 1, 5, 63, 64, 65, 320), 1: REL_COUNTS}
SELF_EDGES = 5                        # s == o triples among the ordinary entities, plus one on the 1025-incidence hub
V_DEC, R_DEC, N_DEC = 301, 237, 3000
V_DEC_WIDE = 521


def _nb(d):
    """The smallest valid block count of d: the encoder in front of the decoder has to exist (d / nb a compiled size)."""
    for nb in range(1, MAX_BLOCKS + 1):
        if d % nb == 0 and d // nb in BLOCK_SIZES:
            return nb
    raise ValueError(d)


def _case(d, R=R_DEC, tag="", rate=None, n=N_DEC, saturate=None, seed=None):
    name = "dec_d%d%s" % (d, tag)
    # W_relation has V rows (oracle.init_params, as the reference's): R > 237 needs more entities than V_DEC
    return dict(name=name, V=V_DEC if R <= R_DEC else V_DEC_WIDE, R=R, d=d, L=1, kind="block", nb=_nb(d), n=n, rate=rate, saturate=saturate,
                seed=seed if seed is not None else 5000 + d + R)


DECODER_GRID = [
    # vec4: T 1 and one partial band; T 1 at its bound (8 bands, one pass); T 2 (9 bands, two passes); the shipped d;
    # T 2 at its bound; T 4 (17 bands); T 4 at its bound; unfused <4> (33 bands, three column passes of k_dec_rel_partial)
    _case(20), _case(256), _case(260), _case(500), _case(512), _case(516), _case(1024), _case(1028),
    # scalar: T 1 / tpr 64 (9 and its bound 63), T 2 / tpr 128 (66 and 126), T 4 / tpr 256 (130 and 255),
    # unfused <1> (258, and 1030 = nine column passes)
    _case(9), _case(63), _case(66), _case(126), _case(130), _case(255), _case(258), _case(1030),
    # the line form's relation band: R = 512 is exactly 64 KB of LDS, R = 513 reads it from global memory
    _case(20, R=512, tag="_R512"), _case(20, R=513, tag="_R513"), _case(260, R=512, tag="_R512"),
    _case(260, R=513, tag="_R513"), _case(1028, R=513, tag="_R513"),
    # W_relation scaled until energies pass |x| = 90: sigmoid saturation, log1pf(__expf(-|x|)) underflow, 1/(1+ex) - 1
    _case(20, tag="_sat", saturate=150.0),
    # batches the device negative sampler tiled: rate 10 (11 copies), rate 1, rate 0 (one copy, still the tiled path),
    # and a single triple (period 1: decoded as an ordinary batch)
    _case(20, tag="_rate10", rate=10, n=1500), _case(66, tag="_rate1", rate=1, n=1500),
    _case(20, tag="_rate0", rate=0, n=N_DEC), _case(20, tag="_n1", rate=10, n=1),
    # the tiled order at every other energy cell (rate 1: TILED_REL_COUNTS[2]): scalar T 1 / T 4, the unfused <1>, vec4 T 2
    # (two band passes) and T 4 (three), the unfused <4> (five band passes, k_dec_rel_partial in the tiled order)
    _case(9, tag="_rate1", rate=1, n=1500), _case(130, tag="_rate1", rate=1, n=1500),
    _case(258, tag="_rate1", rate=1, n=1500), _case(260, tag="_rate1", rate=1, n=1500),
    _case(516, tag="_rate1", rate=1, n=1500), _case(1028, tag="_rate1", rate=1, n=1500),
]

DECODER_CASES = {c["name"]: c for c in DECODER_GRID}

# the train-step subset: scalar T 2 / T 4 / unfused, vec4 at two and at five band passes, the global relation band
TRAIN_STEP_CASES = ("dec_d66", "dec_d255", "dec_d258", "dec_d260", "dec_d1028", "dec_d260_R513")


def rel_counts(case):
    """Triples of relation r < 7 among the case's batch (its first copies when tiled)."""
    return TILED_REL_COUNTS[copies(case)] if case.get("rate") is not None else REL_COUNTS


def case_batch(case):
    """The case's batch: n triples whose entities e < 7 and relations r < 7 have exactly the counts above (random ids
    >= 7 fill the rest), SELF_EDGES s == o triples, and labels Y (a third positive; None for a batch the sampler tiles,
    which writes its own)."""
    V, R, n = case["V"], case["R"], case["n"]
    rng = np.random.RandomState(case["seed"])
    if n == 1:
        return np.array([[7, 7, 8]], np.int32), None
    rc = rel_counts(case)
    rel = np.concatenate([np.repeat(np.arange(len(rc)), rc), rng.randint(len(rc), R, n - sum(rc))])
    ent = np.concatenate([np.repeat(np.arange(len(ENTITY_COUNTS)), ENTITY_COUNTS),
                          rng.randint(len(ENTITY_COUNTS), V, 2 * n - sum(ENTITY_COUNTS))])
    assert len(rel) == n and len(ent) == 2 * n
    rel, ent = rng.permutation(rel), rng.permutation(ent)
    X = np.stack([ent[0::2], rel, ent[1::2]], 1).astype(np.int32)
    ne = len(ENTITY_COUNTS)
    # s == o without changing a count: rows (a, r, b) and (c, r', a) become (a, r, a) and (c, r', b) -- objects swapped
    plain = np.where((X[:, 0] >= ne) & (X[:, 2] >= ne) & (X[:, 0] != X[:, 2]))[0]
    made = 0
    for i in plain:
        if made == SELF_EDGES:
            break
        a, b = X[i, 0], X[i, 2]
        if a == b:
            continue
        j = [k for k in np.where(X[:, 2] == a)[0] if X[k, 0] != a]
        if not j:
            continue
        X[j[0], 2], X[i, 2] = b, a
        made += 1
    # and one on the hub: (6, r, x) and (y, r', 6) -> (6, r, 6) and (y, r', x)
    hub = ne - 1
    i = np.where((X[:, 0] == hub) & (X[:, 2] != hub))[0][0]
    j = np.where((X[:, 2] == hub) & (X[:, 0] != hub))[0][0]
    X[j, 2], X[i, 2] = X[i, 2], hub
    Y = None
    if case.get("rate") is None:
        Y = (rng.rand(n) < 1.0 / 3).astype(np.float32)
    return X, Y


def host_tiled(batch, rate, V, seed):
    """NegativeSampler.transform's layout (code/common/auxilliaries.py:13-33) on the host: the batch tiled rate + 1
    times, one side of every later row replaced by a uniform entity; labels 1 for the first copy."""
    rng = np.random.RandomState(seed)
    n = len(batch)
    X = np.tile(batch, (rate + 1, 1))
    side = rng.rand(n * rate) < 0.5
    ent = rng.randint(0, V, n * rate)
    neg = X[n:]
    neg[side, 2] = ent[side]
    neg[~side, 0] = ent[~side]
    Y = np.zeros(n * (rate + 1), np.float32)
    Y[:n] = 1
    return X.astype(np.int32), Y


# ----------------------------------------------------------------------------- row weights
# decoder_compute launches k_dec_energy_rel<VEC, T, WEIGHTED> / k_dec_energy<VEC, WEIGHTED> with WEIGHTED = (row_weights
# != nullptr): every energy cell exists twice.  A weight is read by ROW ID (Wt[m0], Wt[m1], Wt[n]) while the fused kernel
# walks the relation order (permr), which for a tiled batch is another order again: the weighted cells are held at both.
def is_tiled(case):
    """decoder.hip:1118-1119: decoder_prepare orders a batch the sampler wrote by its first copies when its period is > 1
    (rate 0, a single copy, included)."""
    return case.get("rate") is not None and case["n"] > 1


def weighted_cell_of(case, weighted=True):
    """(energy cell, entity-gradient cell, WEIGHTED): decoder.hip:1192, 1204 -- `row_weights == nullptr` picks the plain
    instantiation of the same cell."""
    return energy_cell(case["d"]), entity_cell(case["d"], case["R"]), bool(weighted)


def weighted_energy_cell(case):
    """The entry of WEIGHTED_ENERGY_CELLS a weighted run of the case executes."""
    return energy_cell(case["d"]), "tiled" if is_tiled(case) else "plain"


WEIGHTED_ENERGY_CELLS = [(cell, order) for cell in ENERGY_CELLS for order in ("plain", "tiled")]

# one untiled case per energy cell, the saturated energies, the global relation band, and every batch the sampler tiled
WEIGHTED_CASES = ("dec_d20", "dec_d260", "dec_d516", "dec_d1028", "dec_d9", "dec_d66", "dec_d130", "dec_d258",
                  "dec_d20_sat", "dec_d260_R513") + \
    tuple(c["name"] for c in DECODER_GRID if is_tiled(c))

# batches with relation rows behind the entity rows (rgcn_negative_sample_relation_device: N = n (rate + 1 + m), the
# general path of decoder_prepare): scalar T 2, vec4 T 2, the unfused <4>
RELATION_ROW_CASES = ("dec_d66_rate1", "dec_d260_rate1", "dec_d1028_rate1")
RELATION_ROW_RATE, RELATION_ROW_M = 1, 2

HIGH = 2.5                            # a weight above it is one of the constructed `large` ones


def relation_order(rel, period=None):
    """permr (decoder.hip:66-81, 1135): the triples sorted by relation, stably; a tiled batch has only its first `period`
    rows sorted, with the copies p + period, p + 2 period, ... of row p directly behind it."""
    rel = np.asarray(rel)
    if period is None:
        return np.argsort(rel, kind="stable")
    first = np.argsort(rel[:period], kind="stable")
    return (first[:, None] + period * np.arange(len(rel) // period)[None, :]).reshape(-1)


def relation_segments(rel, order):
    """[(relation, rows in relation-sort order)] of the relations that have a triple."""
    rs = np.asarray(rel)[order]
    cut = np.flatnonzero(np.diff(rs)) + 1
    return [(int(rs[a]), order[a:b]) for a, b in zip(np.r_[0, cut], np.r_[cut, len(rs)])]


def lone_rows(rows):
    """k_dec_energy_rel's walk over one relation's rows (decoder.hip:764-765, 791-793): chunks of kDecChunk, wave w of a
    chunk takes its triples w, w + 4, w + 8, ... two per turn.  A wave with an odd number of them takes its last one
    alone (`two` false, w1 = 0.f).  Returns, per chunk, the rows taken alone."""
    out = []
    for lo in range(0, len(rows), CHUNK):
        chunk = rows[lo:lo + CHUNK]
        mine = [chunk[w::4] for w in range(4)]
        out.append([int(m[-1]) for m in mine if len(m) % 2 == 1])
    return out


def entity_rows(X, e):
    X = np.asarray(X).reshape(-1, 3)
    return np.flatnonzero((X[:, 0] == e) | (X[:, 2] == e))


def case_weights(case, N, X=None):
    """float32 [N] row weights for the decoded batch of a case (N = n x copies), BUILT so that a wrong index shows:

      * uniform in [0, 3) from the case's seed; a seventh of the rows exactly 0, another seventh exactly 1 -- copy j of
        triple g is 0 / 1 when (a_g + j) mod 7 is 0 / 1, a_g drawn per triple, so that the weights of the copies of a
        triple are pairwise different (up to 7 copies; with more, two zeros or two ones of a triple are 7 copies apart and
        everything else is pairwise different);
      * the last triple in relation-sort order of every relation with an odd count is above HIGH;
      * every relation r < 7 with at least two triples holds an exact 0 and a weight above HIGH, and every chunk of it in
        which a wave takes a triple alone (lone_rows) has such a triple above HIGH;
      * every entity e < 7 that at least two rows touch holds a row of weight 0 and one above HIGH.

    Without X the relation of row i is that of row i mod n of case_batch (what the entity samplers keep) and the entities
    are those of the first copies, which they keep too; the order is the tiled one for a tiled case.  With X (a batch whose
    later rows changed their relation: the relation rows) relations, entities and the general order are taken from it."""
    n = case["n"]
    assert N % n == 0, (N, n)
    k = N // n
    if X is None:
        batch, _ = case_batch(case)
        assert k == 1 or case.get("rate") is not None
        rel, ents = np.tile(batch[:, 1], k), batch
        order = relation_order(rel, n if is_tiled(case) else None)
    else:
        X = np.asarray(X).reshape(N, 3)
        rel, ents = X[:, 1], X
        order = relation_order(rel)
    rng = np.random.RandomState(case["seed"] + 100003)
    w = (rng.rand(N) * 3.0).astype(np.float32)
    kind = (np.tile(rng.randint(0, 7, n), k) + np.arange(N) // n) % 7
    w[kind == 0] = 0.0
    w[kind == 1] = 1.0
    pinned = np.zeros(N, bool)

    def high(rows):
        """a row of `rows` above HIGH: one that is already, else the first free one is made so"""
        have = [i for i in rows if w[i] > HIGH]
        free = [i for i in rows if not pinned[i]]
        assert have or free, (case["name"], "no free row for a large weight")
        i = have[0] if have else free[0]
        if not have:
            w[i] = np.float32(HIGH + 0.005 + 0.49 * rng.rand())
        pinned[i] = True

    def zero(rows):
        have = [i for i in rows if w[i] == 0]
        free = [i for i in rows if not pinned[i] and not (w[i % n::n] == 0).any()]
        assert have or free, (case["name"], "no free row for a zero weight")
        i = have[0] if have else free[0]
        w[i] = 0.0
        pinned[i] = True

    segments = relation_segments(rel, order)
    for r, rows in segments:
        if len(rows) % 2 == 1:
            high(rows[-1:])
    for r, rows in segments:
        if r < len(REL_COUNTS) and len(rows) >= 2:
            high(rows)
            zero(rows)
            for alone in lone_rows(rows):
                if alone:
                    high(alone)
    for e in range(len(ENTITY_COUNTS)):
        rows = entity_rows(ents, e)
        if len(rows) >= 2:
            high(rows)
            zero(rows)
    return w
