"""Negative sampling (reference: code/common/auxilliaries.py).

`NegativeSampler.transform` (:13-33): the batch is tiled (rate + 1) times; the first copy keeps label 1,
every further row gets label 0 and either its object (fair coin = 1) or its subject replaced by a uniformly
drawn entity.  Row (i, j) of the reference's double loop reads `choices[i + j*size]`, `values[i + j*size]`
and writes row `size + i + j*size` — one draw per negative row, in row order — so the vectorised form below
is the same function of the same random streams (`np.random.binomial` then `np.random.randint`).
Corrupted triples are NOT checked against known positives (that is `transform_exclusive`, which no
BASELINE setting calls; `[General] ExclusiveNegativeSampling=Yes` selects it, on the host and on the device).

`relation_rate = m > 0` (`[General] RelationNegativeSampleRate`, not in the reference): both transforms append m further
copies of the batch with label 0 whose RELATION is replaced by one of the `relation_count - 1` others, uniformly -- the
distribution of the device's k_negative_sample_relation, from numpy's stream.  They are drawn after the entity draws, so
with m = 0 the generator is consumed exactly as before.

`transform_typed` (`[General] TypeConstrainedNegatives=Yes`, not in the reference): the entity corruptions are drawn from
the entities `set_type_sets`' triples have seen in that slot of the row's relation, uniformly over the members other than
the row's own entity -- the decision of the device's k_negative_sample_typed (csrc/negative_typed.h) from numpy's stream:
a list with fewer than two members, or with no member but the row's own, is open (all entities); `exclusive` redraws known
positives inside the list up to max_relation_draws times, then scans the list, then falls open.

`reciprocal=True` (`[Decoder] ReciprocalRelations=Yes`, not in the reference): `transform_reciprocal` runs behind whichever
transform drew the rows, relation rows included -- the pass of the device's k_reciprocal_rows
(csrc/negative_reciprocal.h) with the transform's own coin: an entity corruption whose SUBJECT was replaced takes the
relation r + R, and the inverse positives (s, r + R, o), label 1, follow the last row.  It draws nothing."""
import numpy as np


class NegativeSampler(object):
    negative_sample_rate = None
    n_entities = None

    relation_rate = 0
    relation_count = None
    max_relation_draws = 32         # RGCN_NEG_MAX_DRAWS: then the first free relation upward, as on the device

    reciprocal = False

    def __init__(self, negative_sample_rate, n_entities, relation_rate=0, relation_count=None, reciprocal=False):
        self.negative_sample_rate = int(negative_sample_rate)
        self.n_entities = int(n_entities)
        self.relation_rate = int(relation_rate)
        if self.relation_rate < 0:
            raise ValueError("relation_rate must not be negative")
        if self.relation_rate > 0 and (relation_count is None or int(relation_count) < 2):
            raise ValueError("relation corruptions need relation_count >= 2")
        self.relation_count = None if relation_count is None else int(relation_count)
        self.reciprocal = bool(reciprocal)
        if self.reciprocal and (self.relation_count is None or 2 * self.relation_count > self.n_entities):
            raise ValueError("ReciprocalRelations needs relation_count with 2 x relation_count <= n_entities: W_relation "
                             "has one row per entity")

    def _other_relations(self, relations, rng):
        """one relation other than its own for every entry: a draw in [0, R - 1), stepped past the own relation"""
        draws = rng.randint(self.relation_count - 1, size=len(relations))
        return (draws + (draws >= relations)).astype(np.int32)

    def transform_reciprocal(self, triplets, indexes, labels, object_side):
        """The reciprocal pass over the rows a transform returned for `triplets` (relation rows included): `object_side`
        is that transform's coin per entity corruption, true where the OBJECT was replaced.  Those rows keep their
        relation, the others take r + R; the inverse positives (s, r + R, o), label 1, are appended.  A relation outside
        [0, R) stays what it is.  The inputs are left unchanged."""
        triplets = np.asarray(triplets).reshape(-1, 3)
        R, n = self.relation_count, len(triplets)
        object_side = np.asarray(object_side).astype(bool)
        if len(object_side) != n * self.negative_sample_rate:
            raise ValueError("one coin per entity corruption is needed")

        def inverse(r):
            return np.where((r >= 0) & (r < R), r + R, r).astype(np.int32)

        out = np.concatenate([np.asarray(indexes, dtype=np.int32), triplets.astype(np.int32)])
        negatives = out[n:n + len(object_side)]
        negatives[~object_side, 1] = inverse(negatives[~object_side, 1])
        out[len(indexes):, 1] = inverse(out[len(indexes):, 1])
        return out, np.concatenate([np.asarray(labels, dtype=np.float32), np.ones(n, dtype=np.float32)])

    def _append_relation_rows(self, triplets, new_indexes, new_labels, rng, exclusive, choices=None):
        """the relation_rate further copies (s, r', o), label 0, behind the rows of transform / transform_exclusive; then,
        under `reciprocal`, the reciprocal pass with the transform's coin `choices`"""
        new_indexes, new_labels = self._relation_rows(triplets, new_indexes, new_labels, rng, exclusive)
        if self.reciprocal:
            return self.transform_reciprocal(triplets, new_indexes, new_labels, choices)
        return new_indexes, new_labels

    def _relation_rows(self, triplets, new_indexes, new_labels, rng, exclusive):
        if self.relation_rate == 0:
            return new_indexes, new_labels
        rows = np.tile(np.asarray(triplets), (self.relation_rate, 1)).astype(np.int32)
        own = rows[:, 1].copy()
        rows[:, 1] = self._other_relations(own, rng)
        if exclusive:
            R = self.relation_count
            for row, r in zip(rows, own):
                known = self.objs.get(row[0], ())
                first, draws = row[1], 1
                while (row[1], row[2]) in known and draws < self.max_relation_draws:
                    row[1] = self._other_relations(np.array([r]), rng)[0]
                    draws += 1
                if (row[1], row[2]) in known:        # every draw was known: scan; none free: the first draw stays
                    free = [e % R for e in range(row[1] + 1, row[1] + R) if e % R != r and (e % R, row[2]) not in known]
                    row[1] = free[0] if free else first
        return (np.concatenate([new_indexes, rows]),
                np.concatenate([new_labels, np.zeros(len(rows), dtype=np.float32)]))

    def transform(self, triplets, rng=None):
        """`rng`: a numpy RandomState to draw from instead of the global one (background batch producers)."""
        rng = np.random if rng is None else rng
        triplets = np.asarray(triplets)
        size_of_batch = len(triplets)
        number_to_generate = size_of_batch * self.negative_sample_rate
        new_labels = np.zeros(size_of_batch * (self.negative_sample_rate + 1), dtype=np.float32)
        new_indexes = np.tile(triplets, (self.negative_sample_rate + 1, 1)).astype(np.int32)
        new_labels[:size_of_batch] = 1
        choices = rng.binomial(1, 0.5, number_to_generate).astype(bool)
        values = rng.randint(self.n_entities, size=number_to_generate)
        negatives = new_indexes[size_of_batch:]
        negatives[choices, 2] = values[choices]
        negatives[~choices, 0] = values[~choices]
        return self._append_relation_rows(triplets, new_indexes, new_labels, rng, False, choices)

    min_typed_candidates = 2        # RGCN_TYPED_MIN_CANDIDATES
    typed_open = 0                  # rows transform_typed drew over all entities, so far

    def set_type_sets(self, triplets):
        """domain(r) / range(r) of `triplets`: (subjects by relation, objects by relation), each a sorted array"""
        subjects, objects = {}, {}
        for s, r, o in np.asarray(triplets):
            subjects.setdefault(int(r), set()).add(int(s))
            objects.setdefault(int(r), set()).add(int(o))
        self.type_lists = ({r: np.array(sorted(v), dtype=np.int64) for r, v in subjects.items()},
                           {r: np.array(sorted(v), dtype=np.int64) for r, v in objects.items()})

    def transform_typed(self, triplets, rng=None, exclusive=False):
        """As `transform`, every corruption from the type list of its (side, relation); `exclusive`: known positives
        (set_known_positives) are redrawn.  `rng` as in `transform`."""
        rng = np.random if rng is None else rng
        triplets = np.asarray(triplets)
        size_of_batch = len(triplets)
        number_to_generate = size_of_batch * self.negative_sample_rate
        new_labels = np.zeros(size_of_batch * (self.negative_sample_rate + 1), dtype=np.float32)
        new_indexes = np.tile(triplets, (self.negative_sample_rate + 1, 1)).astype(np.int32)
        new_labels[:size_of_batch] = 1
        choices = rng.binomial(1, 0.5, number_to_generate)
        for k in range(number_to_generate):
            row = new_indexes[size_of_batch + k]
            coin = int(choices[k])
            col = 2 if coin else 0
            s, r, o = int(row[0]), int(row[1]), int(row[2])
            if coin:
                def known(e):
                    return (r, e) in self.objs.get(s, ())
            else:
                def known(e):
                    return (r, e) in self.subs.get(o, ())
            L = self.type_lists[coin].get(r)
            done = False
            if L is not None and len(L) >= self.min_typed_candidates:
                own = o if coin else s
                at = int(np.searchsorted(L, own))
                p = at if at < len(L) and L[at] == own else -1
                n = len(L) - (1 if p >= 0 else 0)
                if n >= 1:
                    for _ in range(self.max_relation_draws if exclusive else 1):
                        c = int(rng.randint(n))
                        c += 1 if p >= 0 and c >= p else 0
                        if not exclusive or not known(int(L[c])):
                            done = True
                            break
                    if not done:            # every draw was known: the first other member that is not, upward from the last
                        for _ in range(1, len(L)):
                            c = 0 if c + 1 == len(L) else c + 1
                            if c != p and not known(int(L[c])):
                                done = True
                                break
                    if done:
                        row[col] = L[c]
            if not done:                    # open: the plain (or the exclusive) draw over all entities
                self.typed_open += 1
                row[col] = rng.randint(self.n_entities)
                while exclusive and known(int(row[col])):
                    row[col] = rng.randint(self.n_entities)
        return self._append_relation_rows(triplets, new_indexes, new_labels, rng, exclusive, choices)

    def set_known_positives(self, triplets):
        self.objs, self.subs = {}, {}
        for s, r, o in np.asarray(triplets):
            self.objs.setdefault(s, set()).add((r, o))
            self.subs.setdefault(o, set()).add((r, s))

    def transform_exclusive(self, triplets, rng=None):
        """As `transform`, redrawing every corruption that is a known positive (:48-70).  `rng` as in `transform`;
        without it the draws come from the global generator, in the reference's order."""
        rng = np.random if rng is None else rng
        triplets = np.asarray(triplets)
        size_of_batch = len(triplets)
        number_to_generate = size_of_batch * self.negative_sample_rate
        new_labels = np.zeros(size_of_batch * (self.negative_sample_rate + 1), dtype=np.float32)
        new_indexes = np.tile(triplets, (self.negative_sample_rate + 1, 1)).astype(np.int32)
        new_labels[:size_of_batch] = 1
        choices = rng.binomial(1, 0.5, number_to_generate)
        for k in range(number_to_generate):
            row = new_indexes[size_of_batch + k]
            if choices[k]:
                row[2] = rng.randint(self.n_entities)
                while (row[1], row[2]) in self.objs.get(row[0], ()):
                    row[2] = rng.randint(self.n_entities)
            else:
                row[0] = rng.randint(self.n_entities)
                while (row[1], row[0]) in self.subs.get(row[2], ()):
                    row[0] = rng.randint(self.n_entities)
        return self._append_relation_rows(triplets, new_indexes, new_labels, rng, True, choices)
