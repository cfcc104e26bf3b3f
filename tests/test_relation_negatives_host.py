"""The relation corruptions without a GPU: the host-and-device decision text (csrc/negative_relation.h) under
AddressSanitizer and UndefinedBehaviorSanitizer against the numpy mirror (tests/relation_negatives_reference.py), the
mirror's properties, the numpy port in common/auxilliaries.py, the settings key on the four paths of make_transform and
Metric=RelationMRR."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exclusive_negatives_reference as ent
import relation_negatives_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(ref.CASES)


# ---- 1. the sanitizer driver against the mirror --------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("negative_relation")
    exe = str(tmp / "negative_relation_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "negative_relation_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = []
    for name in NAMES:
        c = ref.case(name)
        for mode in (0, 1):
            lines.append("case %s_%d %d %d %d %d %d %d %d" % (name, mode, c["V"], c["R"], c["relation_rate"], mode, c["seed"],
                                                             len(c["known"]), len(c["batch"])))
            lines += ["%d %d %d" % tuple(row) for row in c["known"].tolist() + c["batch"].tolist()]
    path = tmp / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:] + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.splitlines()
    assert out[-1] == "negative_relation_driver: ok"
    cases, cur = {}, None
    for line in out[:-1]:
        w = line.split()
        if w[0] == "case":
            cur = cases[w[1]] = {"status": int(w[3]), "nkeys": int(w[5]), "rows": []}
        elif w[0] == "row":
            cur["rows"].append([int(x) for x in w[1:]])
        elif w[0] == "end":
            cur["unresolved"] = int(w[3])
    return cases


@pytest.mark.parametrize("mode", [0, 1], ids=["plain", "exclusive"])
@pytest.mark.parametrize("name", NAMES)
def test_driver_equals_the_mirror(driver_output, name, mode):
    """every relation row (s, r', o, lookups, unresolved) of the C++ text, bit for bit, in both forms"""
    c = ref.case(name)
    got = driver_output["%s_%d" % (name, mode)]
    m = (c["mirror"] if mode else c["plain"])["relation"]
    assert got["status"] == 0 and got["nkeys"] == len(c["keys"])
    rows = np.array(got["rows"], dtype=np.int64)
    assert rows.shape == (len(c["batch"]) * c["relation_rate"], 5)
    assert np.array_equal(rows[:, :3], m["X"])
    assert np.array_equal(rows[:, 3], m["lookups"])
    assert np.array_equal(rows[:, 4], m["unresolved_rows"].astype(np.int64))
    assert got["unresolved"] == m["unresolved"]
    if not mode:
        assert not rows[:, 3:].any()               # the plain form looks nothing up and leaves nothing unresolved


def test_mirror_constants_are_the_sources():
    """the mirror's draw limit and tags, as the headers spell them; the tags are the entity samplers' neighbours and none
    of theirs"""
    header = open(os.path.join(ROOT, "include", "rgcn.h")).read()
    assert int(re.search(r"#define RGCN_NEG_MAX_DRAWS (\d+)", header).group(1)) == ref.MAX_DRAWS == ent.MAX_DRAWS
    assert int(re.search(r"RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED = (\d+)", header).group(1)) == 21
    assert int(re.search(r"RGCN_ABI_VERSION (\d+)", header).group(1)) == 1
    csrc = os.path.join(ROOT, "relationprediction_amd", "csrc")
    decision = open(os.path.join(csrc, "negative_relation.h")).read()
    code = "\n".join(line.split("//")[0] for line in decision.splitlines())
    tags = ref.TAG_FIRST + ref.TAG_REDRAW
    assert tags == (0x6e6a, 0x6e6b, 0x6e6c, 0x6e6d)
    assert sorted(re.findall(r"0x6e[0-9a-f]{2}u", code)) == ["0x%xu" % t for t in tags]
    assert "RGCN_NEG_MAX_DRAWS" in code and '#include "negative_exclusive.h"' in code
    entity = open(os.path.join(csrc, "negative_exclusive.h")).read() + open(os.path.join(csrc, "decoder.hip")).read()
    assert not any("0x%xu" % t in entity for t in tags)
    assert not set(tags) & set((ent.TAG_COIN,) + ent.TAG_FIRST + ent.TAG_REDRAW)


# ---- 2. properties, on the mirror ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_entity_rows_are_the_existing_samplers(name):
    """rows [0, n (rate + 1)) equal `plain` / `exclusive` of the existing mirror; the relation rows keep s and o, have
    label 0 and never return the row's own relation"""
    c = ref.case(name)
    n, rate, m = len(c["batch"]), c["rate"], c["relation_rate"]
    first = n * (rate + 1)
    Xp, Yp, _ = ent.plain(c["batch"], rate, c["V"], c["seed"])
    e = ent.exclusive(c["keys"], c["batch"], rate, c["V"], c["R"], c["seed"])
    assert np.array_equal(c["plain"]["X"][:first], Xp) and np.array_equal(c["plain"]["Y"][:first], Yp)
    assert np.array_equal(c["mirror"]["X"][:first], e["X"]) and np.array_equal(c["mirror"]["Y"][:first], e["Y"])
    assert c["mirror"]["entity_unresolved"] == e["unresolved"] and c["plain"]["entity_unresolved"] == 0
    tiled = np.tile(c["batch"], (m, 1))
    for out in (c["plain"], c["mirror"]):
        X, Y, rel = out["X"], out["Y"], out["relation"]
        assert len(X) == len(Y) == n * (1 + rate + m) and (Y[first:] == 0).all()
        assert np.array_equal(X[first:][:, [0, 2]], tiled[:, [0, 2]])
        valid = rel["valid"]
        assert (X[first:][valid, 1] != tiled[valid, 1]).all()
        assert ((X[first:, 1] >= 0) & (X[first:, 1] < c["R"])).all()       # ... and every relation written is one


def test_small_case_redraws_and_stays_out_of_K():
    """V 150, R 9: K covers 10.3 % of the candidate space, so about 165 (sd 12) of the 1,600 relation rows have a known first
    draw: at least 100, so that the device test of this case cannot pass while exercising nothing"""
    c = ref.case("small")
    n, first = len(c["batch"]), len(c["batch"]) * (c["rate"] + 1)
    assert (c["V"], c["R"], n, c["rate"], c["relation_rate"], len(c["known"])) == (150, 9, 800, 2, 2, 20800)
    rel, plain_rel = c["mirror"]["relation"], c["plain"]["relation"]
    K = {tuple(t) for t in c["known"].tolist()}
    plain_known = np.array([tuple(t) in K for t in plain_rel["X"].tolist()])
    assert np.array_equal(plain_known, rel["first_known"])
    assert 100 <= plain_known.sum() <= 260, plain_known.sum()
    # no relation row is in K (none is unresolved), and none is its own positive
    assert rel["unresolved"] == 0 and not any(tuple(t) in K for t in rel["X"].tolist())
    # plain and exclusive differ exactly in the rows whose first draw is known, and there only in column 1
    differs = (rel["X"] != plain_rel["X"]).any(axis=1)
    assert np.array_equal(differs, plain_known)
    assert np.array_equal(rel["X"][:, [0, 2]], plain_rel["X"][:, [0, 2]])
    assert (rel["lookups"][~plain_known] == 1).all() and (rel["lookups"][plain_known] >= 2).all()
    assert not plain_rel["lookups"].any()
    # a function of (K, batch, seed) alone
    args = (c["keys"], c["batch"], c["rate"], c["relation_rate"], c["V"], c["R"])
    assert np.array_equal(ref.sample(*args, c["seed"], True)["X"], c["mirror"]["X"])
    assert not np.array_equal(ref.sample(*args, c["seed"] + 1, True)["X"][first:], c["mirror"]["X"][first:])


def test_two_relations_flip():
    """R = 2: r' = 1 - r for every row, whatever the draw"""
    c = ref.case("two_relations")
    first = len(c["batch"]) * (c["rate"] + 1)
    tiled = np.tile(c["batch"], (c["relation_rate"], 1))
    for out in (c["plain"], c["mirror"]):
        assert np.array_equal(out["X"][first:, 1], 1 - tiled[:, 1])


def test_scan_finds_the_one_free_relation():
    c = ref.case("scan")
    rel = c["mirror"]["relation"]
    assert len(rel["X"]) == 128 and c["R"] == 64 and len(c["known"]) == 62
    assert rel["scanned"].sum() >= 30, rel["scanned"].sum()         # (62/63)^32 = 0.60 of the rows
    assert (rel["X"][:, 1] == 37).all() and rel["unresolved"] == 0
    assert (rel["lookups"][rel["scanned"]] > ref.MAX_DRAWS).all()
    assert (rel["lookups"] <= ref.MAX_DRAWS + c["R"] - 1).all()     # the scan: at most R - 1 lookups
    assert (c["plain"]["relation"]["X"][:, 1] != 0).all()


def test_saturated_rows_keep_their_first_draw_and_are_counted():
    c = ref.case("saturated")
    rel, plain_rel = c["mirror"]["relation"], c["plain"]["relation"]
    assert len(c["known"]) == 63 and rel["unresolved"] == 128 and rel["unresolved_rows"].all()
    assert np.array_equal(rel["X"], plain_rel["X"]) and np.array_equal(rel["X"][:, 1], rel["first"])
    assert c["mirror"]["entity_unresolved"] == 0                    # the entity rows' counter is another


def test_rows_with_an_id_out_of_range():
    """r' = the raw draw of attempt 0 (in range, no skip), no lookup; every other row as if the bad rows were not there"""
    c = ref.case("invalid_rows")
    n, m = len(c["batch"]), c["relation_rate"]
    bad = np.tile(np.isin(np.arange(n), [3, 11, 17]), m)
    for out in (c["plain"], c["mirror"]):
        rel = out["relation"]
        assert np.array_equal(~rel["valid"], bad)
        assert (rel["lookups"][bad] == 0).all() and np.array_equal(rel["X"][bad, 1], rel["first"][bad])
        assert ((rel["first"][bad] >= 0) & (rel["first"][bad] < c["R"] - 1)).all()
    assert (c["mirror"]["relation"]["lookups"][~bad] >= 1).all()


def _chi2(values, free):
    counts = np.array([(values == e).sum() for e in free], dtype=np.float64)
    assert counts.sum() == len(values), "a replacement outside the free ids"
    expected = len(values) / float(len(free))
    return ((counts - expected) ** 2 / expected).sum()


def test_first_draws_are_uniform_over_the_other_relations():
    """attempt-0 candidates at R = 9 over the 8 other relations, for an own relation at the bottom, inside and at the top
    of the range, by the project's margin |chi2 - dof| < 5 sqrt(2 dof)"""
    R, V = 9, 150
    for own in (0, 4, 8):
        batch = np.array([(1, own, 2)] * 2000, dtype=np.int32)
        rel = ref.relation_rows(np.zeros(0, dtype=np.uint64), batch, 2, V, R, 7, False)
        free = [r for r in range(R) if r != own]
        dof = len(free) - 1
        chi2 = _chi2(rel["X"][:, 1], free)
        assert abs(chi2 - dof) < 5 * np.sqrt(2 * dof), (own, chi2, dof)


# ---- 3. the host port ------------------------------------------------------------------------------------------------

def _toy_graph():
    # dense on purpose: 12 entities, 3 relations, 200 of the 432 triples
    rng = np.random.RandomState(1)
    every = np.array([(s, r, o) for s in range(12) for r in range(3) for o in range(12)], dtype=np.int32)
    return every[rng.permutation(len(every))[:200]]


@pytest.mark.parametrize("exclusive", [False, True])
def test_host_port_layout_labels_and_seed(exclusive):
    from relationprediction_amd.common import auxilliaries
    train = _toy_graph()
    ns = auxilliaries.NegativeSampler(3, 12, relation_rate=2, relation_count=3)
    ns.set_known_positives(train)
    fn = ns.transform_exclusive if exclusive else ns.transform
    batch, n = train[:40], 40
    X, Y = fn(batch, np.random.RandomState(5))
    assert X.shape == (n * 6, 3) and X.dtype == np.int32 and Y.shape == (n * 6,) and Y.dtype == np.float32
    assert (Y[:n] == 1).all() and (Y[n:] == 0).all() and np.array_equal(X[:n], batch)
    rel = X[n * 4:]
    tiled = np.tile(batch, (2, 1))
    assert np.array_equal(rel[:, [0, 2]], tiled[:, [0, 2]]) and (rel[:, 1] != tiled[:, 1]).all()
    assert ((rel[:, 1] >= 0) & (rel[:, 1] < 3)).all() and len(set(rel[:, 1].tolist())) == 3
    assert (X[n:n * 4, 1] == np.tile(batch, (3, 1))[:, 1]).all()         # the entity rows keep their relation
    X2, Y2 = fn(batch, np.random.RandomState(5))
    X3, _ = fn(batch, np.random.RandomState(6))
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2) and not np.array_equal(X, X3)
    if exclusive:
        # a row whose other two relations are both known keeps its first draw (the device's unresolved rows)
        K = {tuple(t) for t in train.tolist()}
        for row, own in zip(rel.tolist(), tiled[:, 1].tolist()):
            others = [(row[0], r, row[2]) in K for r in range(3) if r != own]
            assert tuple(row) not in K or all(others)


@pytest.mark.parametrize("exclusive", [False, True])
def test_host_port_with_rate_zero_is_todays(exclusive):
    """relation_rate = 0: the output and the generator's state afterwards are those of a sampler built the old way"""
    from relationprediction_amd.common import auxilliaries
    train = _toy_graph()
    old, new = auxilliaries.NegativeSampler(3, 12), auxilliaries.NegativeSampler(3, 12, relation_rate=0, relation_count=3)
    for ns in (old, new):
        ns.set_known_positives(train)
    name = "transform_exclusive" if exclusive else "transform"
    ra, rb = np.random.RandomState(9), np.random.RandomState(9)
    a, b = getattr(old, name)(train[:50], ra), getattr(new, name)(train[:50], rb)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) == 200
    assert ra.randint(0, 2 ** 31 - 1) == rb.randint(0, 2 ** 31 - 1)
    # the relation rows are drawn AFTER the entity draws: the front of a batch with them is the batch without them
    with_rows = auxilliaries.NegativeSampler(3, 12, relation_rate=1, relation_count=3)
    with_rows.set_known_positives(train)
    c = getattr(with_rows, name)(train[:50], np.random.RandomState(9))
    assert np.array_equal(c[0][:200], a[0]) and len(c[0]) == 250
    with pytest.raises(ValueError):
        auxilliaries.NegativeSampler(3, 12, relation_rate=1, relation_count=1)
    with pytest.raises(ValueError):
        auxilliaries.NegativeSampler(3, 12, relation_rate=1)


# ---- 4. the setting --------------------------------------------------------------------------------------------------

class _Settings(dict):
    pass


class _Encoder(object):
    def __init__(self, graph=True):
        self.graph = graph

    def needs_graph(self):
        return self.graph


@pytest.mark.parametrize("value,expected", [(None, 0), ("0", 0), ("2", 2), (3, 3), (" 1 ", 1)])
def test_setting_is_parsed(value, expected):
    from relationprediction_amd import train as train_module
    settings = _Settings(RelationCount=3)
    if value is not None:
        settings["RelationNegativeSampleRate"] = value
    assert train_module.relation_negative_sample_rate(settings) == expected


@pytest.mark.parametrize("value", ["-1", "1.5", "two", "", "Yes", 1.0, True, "+2"])
def test_a_bad_setting_value_is_refused(value):
    from relationprediction_amd import train as train_module
    settings = _Settings(NegativeSampleRate=5, EntityCount=12, RelationCount=3, GraphSplitSize=0.5,
                         RelationNegativeSampleRate=value)
    with pytest.raises(ValueError, match="RelationNegativeSampleRate"):
        train_module.make_transform(_toy_graph(), settings, _Encoder())


def test_one_relation_is_refused_at_start_up():
    from relationprediction_amd import train as train_module
    settings = _Settings(NegativeSampleRate=5, EntityCount=12, RelationCount=1, GraphSplitSize=0.5,
                         RelationNegativeSampleRate="2")
    with pytest.raises(ValueError, match="two relations"):
        train_module.make_transform(_toy_graph(), settings, _Encoder())
    settings["RelationNegativeSampleRate"] = "0"                  # rate 0 asks nothing of the relation count
    train_module.make_transform(_toy_graph(), settings, _Encoder())


@pytest.mark.parametrize("rate", [0, 2])
def test_all_four_paths_carry_the_rate(rate):
    """host: the rows are in X; device negatives, device dropout and device sampler: the batch objects carry the rate"""
    from relationprediction_amd import train as train_module
    from relationprediction_amd.optimization.optimize import DeviceMinibatch, DeviceNegatives
    train = _toy_graph()
    settings = _Settings(NegativeSampleRate=5, EntityCount=12, RelationCount=3, GraphSplitSize=0.5)
    if rate:
        settings["RelationNegativeSampleRate"] = str(rate)
    n = len(train)
    split, X, Y = train_module.make_transform(train, settings, _Encoder()).seeded(train, 1)
    assert len(X) == len(Y) == n * (6 + rate) and (Y[n:] == 0).all()
    assert (X[n * 6:, 1] != np.tile(train, (rate, 1))[:, 1]).all()
    assert np.array_equal(X[n * 6:][:, [0, 2]], np.tile(train, (rate, 1))[:, [0, 2]])
    a = train_module.make_transform(train, settings, _Encoder(), device_negatives=True).seeded(train, 1)
    b = train_module.make_transform(train, settings, _Encoder(), device_negatives=True, device_dropout=True).seeded(train, 1)
    sampled = _Settings(settings, GraphBatchSize=100)
    c = train_module.make_transform(train, sampled, _Encoder(), device_negatives=True, device_dropout=True,
                                    device_sampler=True).seeded(train, 1)
    d = train_module.make_transform(train, settings, _Encoder(graph=False), device_negatives=True).seeded(train, 1)
    assert isinstance(a, DeviceNegatives) and isinstance(b, DeviceMinibatch) and isinstance(c, DeviceMinibatch)
    assert isinstance(d, DeviceNegatives) and c.sample is not None and b.sample is None
    assert [x.relation_rate for x in (a, b, c, d)] == [rate] * 4
    # the batch objects default to 0, and the optimizer hands a nonzero rate on behind `known`
    assert DeviceNegatives(None, train, 5).relation_rate == 0 and DeviceMinibatch(train, 10, 1, 5).relation_rate == 0
    from relationprediction_amd.optimization.optimize import HipOptimizer
    calls = []

    class _Model(object):
        def device_train_step_negatives(self, *args):
            calls.append(args)
    opt = HipOptimizer.__new__(HipOptimizer)
    opt.model = _Model()
    opt.update_from_batch(a, 3)
    assert len(calls[0]) == (6 if rate else 4) and (not rate or calls[0][4:] == (None, rate))


# ---- 5. the metric ---------------------------------------------------------------------------------------------------

TRIPLES = np.array([[0, 0, 1], [0, 1, 1], [0, 0, 1], [3, 1, 0], [2, 0, 1], [1, 2, 0]])


class _RankModel(object):
    """device_relation_ranks stand-in: scripted ranks, handed out in order, over and over"""

    def __init__(self, raw, filtered, unresolved=0):
        self.raw, self.filtered, self.unresolved = np.asarray(raw), np.asarray(filtered), unresolved
        self.test_graph = "graph"
        self.calls = 0

    def device_relation_ranks(self, graph, triples, ptr, idx):
        self.calls += 1
        return self.raw[:len(triples)].astype(np.int32), self.filtered[:len(triples)].astype(np.int32)

    def device_ranks(self, *args):
        raise AssertionError("Metric=RelationMRR asks no entity-side ranks")

    def device_negative_unresolved(self):
        return 0

    def device_negative_relation_unresolved(self):
        return self.unresolved


def _scorer(model):
    from relationprediction_amd.common import evaluation
    scorer = evaluation.Scorer({'Metric': 'RelationMRR'})
    scorer.register_data(TRIPLES)
    scorer.register_degrees(TRIPLES)
    scorer.finalize_frequency_computation(TRIPLES)
    scorer.register_model(model)
    return scorer


def test_metric_loads_a_dataset_and_auc_is_still_refused(tmp_path):
    from relationprediction_amd import train
    from relationprediction_amd.common import evaluation
    (tmp_path / "entities.dict").write_text("0\ta\n1\tb\n2\tc\n")
    (tmp_path / "relations.dict").write_text("0\tr\n1\tq\n")
    (tmp_path / "train.txt").write_text("a\tr\tb\nb\tq\tc\n")
    (tmp_path / "valid.txt").write_text("a\tq\tc\n")
    (tmp_path / "test.txt").write_text("c\tq\ta\n")
    splits, entities, relations = train.load_dataset(str(tmp_path), metric='RelationMRR')
    assert splits['valid'].tolist() == [[0, 1, 2]] and splits['test'].tolist() == [[2, 1, 0]]   # valid.txt / test.txt
    assert len(entities) == 3 and len(relations) == 2
    with pytest.raises(NotImplementedError, match="MRR"):
        train.load_dataset(str(tmp_path), metric='AUC')
    with pytest.raises(NotImplementedError):
        evaluation.Scorer({'Metric': 'AUC'}).compute_scores(TRIPLES)


def test_compute_scores_routes_the_metric():
    from relationprediction_amd.common import evaluation
    test = np.array([[0, 0, 1], [3, 1, 0], [2, 0, 1], [1, 2, 0], [0, 1, 1]])
    model = _RankModel(raw=[1, 2, 4, 3, 10], filtered=[1, 1, 2, 3, 5])
    score = _scorer(model).compute_scores(test)
    assert isinstance(score, evaluation.MrrScore) and score.pointer == len(test) and model.calls == 1
    results = score.get_summary().results
    assert results['Raw']['MRR'] == pytest.approx(np.mean([1, 1 / 2, 1 / 4, 1 / 3, 1 / 10]))
    assert results['Filtered']['MRR'] == pytest.approx(np.mean([1, 1, 1 / 2, 1 / 3, 1 / 5]))
    assert results['Filtered']['H@1'] == pytest.approx(2 / 5)


@pytest.mark.parametrize("unresolved", [0, 7])
def test_validation_function_returns_the_filtered_relation_mrr(capsys, unresolved):
    """early stopping on the validation split's filtered relation MRR; the test split's table in the MRR / H@n format; the
    relation counter on a line of its own when it is nonzero"""
    from relationprediction_amd import train
    valid = np.array([[0, 0, 1], [3, 1, 0], [2, 0, 1]])
    test = np.array([[1, 2, 0], [0, 1, 1]])
    model = _RankModel(raw=[2, 2, 4], filtered=[1, 2, 4], unresolved=unresolved)
    fn = train.make_validation_function(_scorer(model), 'RelationMRR', test, model)
    assert fn(valid) == pytest.approx(np.mean([1, 1 / 2, 1 / 4]))
    out = capsys.readouterr().out
    assert "MRR" in out and "H@1" in out and "H@10" in out
    line = [x for x in out.splitlines() if x.startswith("Exclusive relation negative sampling:")]
    assert len(line) == (1 if unresolved else 0) and (not unresolved or " 7 rows" in line[0])
    assert "Exclusive negative sampling:" not in out
