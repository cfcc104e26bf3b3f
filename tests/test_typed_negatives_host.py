"""The type-constrained sampler without a GPU: the host build of the sets and the host-and-device decision text under
AddressSanitizer and UndefinedBehaviorSanitizer against the mirror (tests/typed_negatives_reference.py), the mirror
against Python sets and against the plain and exclusive samplers' mirror, the uniformity of the draws, the settings keys
with their refusals, and the host path of make_transform."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import exclusive_negatives_reference as xref
import typed_negatives_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V, R = 40, 6


def _host_T():
    """relation 0 absent; relation 1 one pair, twice (singleton lists); relation 2 subjects {1, 2} (m = 2) and objects
    {3, 4, 8} (m = 3); relation 3 subjects 0 .. 32 (m = 33); relation 4 objects 0 .. 32 of subject 35; relation R - 1 the
    ids V - 1"""
    t = [(5, 1, 6), (5, 1, 6)]
    t += [(1, 2, 3), (2, 2, 4), (1, 2, 8), (2, 2, 3), (1, 2, 3)]
    t += [(s, 3, (7 * s) % 5 + 10) for s in range(33)]
    t += [(35, 4, o) for o in range(33)]
    t += [(V - 1, R - 1, V - 1), (0, R - 1, V - 1), (V - 1, R - 1, 0)]
    return np.array(t, dtype=np.int32)


def _driver_cases():
    """name -> (rate, seed, exclusive, T, known, batch); small on purpose: every output row is compared"""
    T = _host_T()
    own_rows = np.array([(1, 2, 3), (2, 2, 8), (7, 2, 9), (0, 3, 10), (32, 3, 14), (36, 3, 39), (5, 1, 6), (4, 0, 4),
                         (V - 1, R - 1, V - 1), (0, R - 1, V - 1), (V - 1, R - 1, 0), (35, 4, 32)], dtype=np.int32)
    bad_rows = np.array([(-1, 2, 3), (1, R, 3), (1, 2, V), (1, 2, 3), (2 ** 31 - 1, 3, 1), (1, -5, 3)], dtype=np.int32)
    # every other member known: objects {20, 21, 22} of (10, 0, .) and subjects {10, 11} of (., 0, 20)
    sat_T = np.array([(10, 0, 20), (10, 0, 21), (10, 0, 22), (11, 0, 20)], dtype=np.int32)
    # the scan: 31 of the 32 other objects of (35, 4, .) are known, the free one sits at position 1, own at position 0
    scan_K = np.array([(35, 4, o) for o in [0] + list(range(2, 33))], dtype=np.int32)
    none = np.zeros((0, 3), np.int32)
    return {
        "plain": (4, 11, 0, T, none, own_rows),
        "exclusive": (4, 11, 1, T, T, own_rows),
        "edge_seed": (3, 2 ** 40 + 17, 1, T, T, own_rows),
        "bad_batch_row": (4, 99, 0, T, none, bad_rows),
        "bad_batch_row_exclusive": (4, 99, 1, T, T, bad_rows),
        "bad_T_subject": (2, 5, 0, np.array([(1, 0, 2), (V, 0, 2)], np.int32), none, own_rows[:3]),
        "bad_T_relation": (2, 5, 0, np.array([(1, R, 2)], np.int32), none, own_rows[:3]),
        "bad_T_negative": (2, 5, 0, np.array([(1, 0, -1)], np.int32), none, own_rows[:3]),
        "all_known_goes_open": (6, 21, 1, sat_T, sat_T, np.array([(10, 0, 20)] * 20, dtype=np.int32)),
        "scan_wraps": (8, 33, 1, T, scan_K, np.array([(35, 4, 0)] * 25, dtype=np.int32)),
    }


LIMITS = {                         # name -> (V, R, num_triples, expected status)
    "fb15k_237": (14541, 237, 272115, 0),
    "fb15k": (14951, 1345, 483142, 0),
    "words_2_31": (2 ** 25, 2 ** 10, 10, 5),                   # 2 R ceil(V/32) = 2 * 2^10 * 2^20 = 2^31
    "words_below_2_31": (2 ** 25 - 32, 2 ** 10, 10, 0),
    "partial_word_counts": (2 ** 25 - 31, 2 ** 10, 10, 5),     # ceil: one entity into the last word is a whole word
    "r_2_30": (1, 2 ** 30, 10, 5),
    "triples_2_31": (100, 5, 2 ** 31, 5),
    "triples_2_31_less_1": (100, 5, 2 ** 31 - 1, 0),
}


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("negative_typed")
    exe = str(tmp / "negative_typed_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "negative_typed_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = []
    for name, (v, rel, num, _) in LIMITS.items():
        lines.append("limits %s %d %d %d" % (name, v, rel, num))
    for name, (rate, seed, exclusive, T, known, batch) in _driver_cases().items():
        lines.append("case %s %d %d %d %d %d %d %d %d" % (name, V, R, rate, seed, exclusive, len(T), len(known), len(batch)))
        lines += ["%d %d %d" % tuple(row) for row in T.tolist() + known.tolist() + batch.tolist()]
    path = tmp / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:] + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.splitlines()
    assert out[-1] == "negative_typed_driver: ok"
    limits, cases, cur = {}, {}, None
    for line in out[:-1]:
        w = line.split()
        if w[0] == "limits":
            limits[w[1]] = int(w[2])
        elif w[0] == "case":
            cur = cases[w[1]] = {"status": int(w[3]), "words": int(w[5]), "mask": [], "rows": []}
        elif w[0] in ("ptr", "idx"):
            cur[w[0]] = [int(x) for x in w[1:]]
        elif w[0] == "mask":
            cur["mask"].append([int(x) for x in w[1:]])
        elif w[0] == "row":
            cur["rows"].append([int(x) for x in w[1:]])
        elif w[0] == "end":
            cur["open"], cur["unresolved"] = int(w[3]), int(w[5])
    return limits, cases


def test_driver_limits_are_arithmetic(driver_output):
    """2 R ceil(V/32) >= 2^31 words and 2^31 triples are refused (RGCN_ERR_UNSUPPORTED = 5) from the numbers alone: the
    driver allocates nothing for these lines, and the mirror's Python integers agree"""
    limits, _ = driver_output
    assert limits == {k: v[3] for k, v in LIMITS.items()}
    for name, (v, rel, num, status) in LIMITS.items():
        assert ref.sets_limits(v, rel, num) == status, name


@pytest.mark.parametrize("name", sorted(_driver_cases()))
def test_driver_equals_the_mirror(driver_output, name):
    """the sets (ptr, idx, every mask word) and every output row (s, r, o, label, open, lookups, unresolved) of the C++
    text, bit for bit"""
    _, cases = driver_output
    rate, seed, exclusive, T, known, batch = _driver_cases()[name]
    got = cases[name]
    if name.startswith("bad_T"):
        # RGCN_ERR_INVALID, and what the build was handed is as it was: the earlier sets stay in place
        assert got["status"] == 1 and got["ptr"] == [7] and got["idx"] == [] and got["mask"] == [] and got["rows"] == []
        with pytest.raises(ValueError):
            ref.build_sets(T, V, R)
        return
    sets = ref.build_sets(T, V, R)
    assert got["status"] == 0 and got["words"] == (V + 31) // 32
    assert got["ptr"] == sets["ptr"].tolist() and got["idx"] == sets["idx"].tolist()
    assert got["mask"] == sets["mask"].tolist()
    m = ref.typed(sets, known, batch, rate, seed, bool(exclusive))
    n = len(batch)
    rows = np.array(got["rows"], dtype=np.int64)
    assert rows.shape == (n * (rate + 1), 7)
    assert np.array_equal(rows[:, :3], m["X"])
    assert np.array_equal(rows[:, 3], m["Y"].astype(np.int64))
    assert np.array_equal(rows[n:, 4], m["open"].astype(np.int64)) and (rows[:n, 4] == 0).all()
    assert np.array_equal(rows[n:, 5], m["lookups"]) and np.array_equal(rows[n:, 6], m["unresolved"])
    assert got["open"] == m["open_count"] and got["unresolved"] == m["unresolved_count"]
    neg, coin = m["X"][n:], m["coin"]
    tiled = np.tile(batch, (rate, 1))
    if name in ("plain", "exclusive", "edge_seed"):
        lens = np.diff(sets["ptr"])
        assert sorted(set(lens.tolist())) == [0, 1, 2, 3, 5, 33]             # absent, singleton, m = 2, 3, 33
        # (V = 40: the last word of an open row holds eight bits)
        assert (sets["mask"][[0, R, 1, R + 1], 0] == 0xffffffff).all() and (sets["mask"][[0, R, 1, R + 1], 1] == 0xff).all()
        # rows of the absent relation 0 and of the singleton relation 1 are open, the others typed: never own, in the list
        assert m["open"][np.isin(tiled[:, 1], [0, 1])].all()
        typed_rows = ~m["open"]
        assert typed_rows.any() and not typed_rows[np.isin(tiled[:, 1], [0, 1])].any()
        for row, src, c in zip(neg[typed_rows].tolist(), tiled[typed_rows].tolist(), coin[typed_rows].tolist()):
            e, own = (row[2], src[2]) if c else (row[0], src[0])
            assert e != own and e in ref.candidate_set(sets, int(c), src[1])
        # m = 2 with own inside: the one other member, every time -- unless it is known (K = T knows both), then open
        two = (tiled[:, 1] == 2) & ~coin & np.isin(tiled[:, 0], [1, 2])
        assert two.any()
        if exclusive:
            assert m["open"][two].all()
        else:
            assert (neg[two, 0] == 3 - tiled[two, 0]).all() and not m["open"][two].any()
    if name.startswith("bad_batch_row"):
        tiled_bad = np.tile(np.array([True, True, True, False, True, True]), rate)
        assert m["open"][tiled_bad].all() and (m["lookups"][tiled_bad] == 0).all()
        assert np.array_equal(neg[tiled_bad], xref.plain(batch, rate, V, seed)[0][n:][tiled_bad])
        if not exclusive:
            assert not m["open"][~tiled_bad].any()
    if name == "all_known_goes_open":
        # both sides of (10, 0, 20): every other member is known, the row takes the exclusive decision over all entities
        assert m["open"].all() and m["open_count"] == n * rate and (m["lookups"] > ref.MAX_DRAWS).all()
        K = {tuple(t) for t in known.tolist()}
        assert not any(tuple(t) in K for t in neg.tolist())
        ex = xref.exclusive(xref.build_index(known, V, R), batch, rate, V, R, seed)
        assert np.array_equal(ex["X"], m["X"])
    if name == "scan_wraps":
        obj = coin
        scanned = obj & (m["lookups"] > ref.MAX_DRAWS)
        # (31/32)^32 = 0.36 of the object rows exhaust their draws; the scan runs past the end of L, passes over p = 0
        # and stops at position 1
        assert scanned.sum() >= 10 and (neg[obj, 2] == 1).all() and not m["open"][obj].any()
        assert m["open"][~obj].all()               # the subject list of relation 4 is the singleton {35}


def test_mirror_constants_are_the_sources():
    """the mirror's limits, tags and the header's dependencies, as the sources spell them"""
    import re
    header = open(os.path.join(ROOT, "include", "rgcn.h")).read()
    assert int(re.search(r"#define RGCN_NEG_MAX_DRAWS (\d+)", header).group(1)) == ref.MAX_DRAWS
    assert int(re.search(r"#define RGCN_TYPED_MIN_CANDIDATES (\d+)", header).group(1)) == ref.MIN_CANDIDATES == 2
    assert re.search(r"RGCN_BUF_NEGATIVE_TYPED_OPEN = 28\b", header)
    csrc = os.path.join(ROOT, "relationprediction_amd", "csrc")
    decision = open(os.path.join(csrc, "negative_typed.h")).read()
    for tag in (ref.TAG_COIN,) + ref.TAG_FIRST + ref.TAG_REDRAW:
        assert "0x%xu" % tag in decision
    includes = set(re.findall(r'#include [<"]([^>"]+)[>"]', decision))
    assert includes == {"cstdint", "../../include/rgcn.h", "counter_rng.h", "negative_exclusive.h"}
    assert (ref.GOLDEN, ref.MUL1, ref.MUL2) == (xref.GOLDEN, xref.MUL1, xref.MUL2)
    idx = np.arange(50)
    assert [ref.bits(12345, 0x6e66, int(i)) for i in idx] == xref.drop_bits(12345, 0x6e66, idx).tolist()


# ---- the mirror against Python sets and against the other samplers' mirror ------------------------------------------

@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_mirror_against_python_sets(name):
    c = ref.case(name)
    Vc, Rc, n, rate, sets = c["V"], c["R"], len(c["batch"]), c["rate"], c["sets"]
    subjects, objects = {}, {}
    for s, r, o in c["T"].tolist():
        subjects.setdefault(r, set()).add(s)
        objects.setdefault(r, set()).add(o)
    for r in range(Rc):
        for side, members in ((0, subjects.get(r, set())), (1, objects.get(r, set()))):
            l = side * Rc + r
            assert sets["idx"][sets["ptr"][l]:sets["ptr"][l + 1]].tolist() == sorted(members)
            stands_for = members if len(members) >= 2 else set(range(Vc))
            bits_set = {e for e in range(32 * sets["mask"].shape[1]) if (int(sets["mask"][l, e >> 5]) >> (e & 31)) & 1}
            assert bits_set == stands_for                      # (no pad bit among them)
    K = {tuple(t) for t in c["known"].tolist()}
    tiled = np.tile(c["batch"], (rate, 1)).tolist()
    keys = xref.build_index(c["known"], Vc, Rc)
    others = {False: xref.plain(c["batch"], rate, Vc, c["seed"])[0],
              True: xref.exclusive(keys, c["batch"], rate, Vc, Rc, c["seed"])["X"]}
    for exclusive in (False, True):
        m = c["exclusive" if exclusive else "plain"]
        assert np.array_equal(m["X"][:n], c["batch"]) and (m["Y"][:n] == 1).all() and (m["Y"][n:] == 0).all()
        assert np.array_equal(m["coin"], xref.plain(c["batch"], rate, Vc, c["seed"])[2])      # the plain sampler's coin
        typed_rows = 0
        for j, ((s, r, o), row) in enumerate(zip(tiled, m["X"][n:].tolist())):
            coin = int(m["coin"][j])
            valid = 0 <= s < Vc and 0 <= o < Vc and 0 <= r < Rc
            members = (objects if coin else subjects).get(r, set()) if valid else set()
            own = o if coin else s
            expect_typed = len(members) >= 2 and len(members - {own}) >= 1
            e = row[2] if coin else row[0]
            assert row[1] == r and (row[0] == s if coin else row[2] == o)
            if not m["open"][j]:
                assert expect_typed and e in members and e != own
                assert not exclusive or tuple(row) not in K
                typed_rows += 1
            else:
                # open by its list, or (exclusive) because every other member is known; drawn as the other sampler draws
                assert not expect_typed or (exclusive and all(
                    ((s, r, x) if coin else (x, r, o)) in K for x in members - {own}))
                assert row == others[exclusive][n + j].tolist()
        if rate:
            assert typed_rows >= 0.3 * n * rate and m["open_count"] >= 2 * rate       # both kinds of row are there
        # a function of (T, K, batch, seed) alone
        again = ref.typed(sets, c["known"], c["batch"], rate, c["seed"], exclusive)
        assert np.array_equal(again["X"], m["X"])
    if rate:
        assert not np.array_equal(c["plain"]["X"], c["exclusive"]["X"])              # (some first draws were known)


# ---- uniformity ------------------------------------------------------------------------------------------------------

UNIFORM_SEED = 7


def _chi2(values, free):
    counts = np.array([(values == e).sum() for e in free], dtype=np.float64)
    assert counts.sum() == len(values), "a replacement outside the other members"
    expected = len(values) / float(len(free))
    return ((counts - expected) ** 2 / expected).sum()


def test_typed_draws_are_uniform_over_the_other_members():
    """subject replacements of (16, 3, .) uniform over the 32 other subjects of relation 3, and with the even ones known
    (exclusive) over the 16 odd ones, by the project's margin |chi2 - dof| < 5 sqrt(2 dof)"""
    sets = ref.build_sets(_host_T(), V, R)
    batch = np.array([(16, 3, 12)] * 1500, dtype=np.int32)
    known = np.array([(s, 3, 12) for s in range(0, 33, 2)], dtype=np.int32)
    for exclusive, free in ((False, [s for s in range(33) if s != 16]), (True, list(range(1, 33, 2)))):
        m = ref.typed(sets, known, batch, 8, UNIFORM_SEED, exclusive)
        values = m["X"][len(batch):][~m["coin"], 0]
        assert len(values) > 5000 and not m["open"][~m["coin"]].any()
        dof = len(free) - 1
        chi2 = _chi2(values, free)
        assert abs(chi2 - dof) < 5 * np.sqrt(2 * dof), (exclusive, chi2, dof)


# ---- ranks and top-k of the mirror -----------------------------------------------------------------------------------

def test_typed_ranks_and_topk_of_the_mirror_by_hand():
    sets = ref.build_sets(np.array([(0, 0, 1), (0, 0, 2), (3, 0, 4), (0, 1, 5)], dtype=np.int32), 6, 2)
    energies = np.array([[5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5]], dtype=np.float32)
    queries = np.array([(0, 0, 4), (0, 0, 5)], dtype=np.int32)
    # objects of relation 0: {1, 2, 4}.  Row 0: gold 4, score 1: 1, 2, 4 reach it -> raw 3; filter {1, 0}: only 1 is a
    # candidate -> filtered 3.  Row 1: gold 5 is outside the list and joins it: only 5 reaches -> 1 and 1.
    raw, filt = ref.typed_ranks_from_energies(sets, energies, queries, True, [[1, 0], [5]])
    assert raw.tolist() == [3, 1] and filt.tolist() == [3, 1]
    idx, val = ref.typed_topk_from_energies(sets, energies, queries, True, 4, [[2], []])
    assert idx.tolist() == [[1, 4, -1, -1], [4, 2, 1, -1]]
    assert val[0].tolist() == [4.0, 1.0, -np.inf, -np.inf]
    # relation 1 has singleton lists: open, all six entities
    idx, _ = ref.typed_topk_from_energies(sets, energies[:1], np.array([(0, 1, 0)], dtype=np.int32), True, 6)
    assert idx.tolist() == [[0, 1, 2, 3, 4, 5]]


# ---- settings and the host path --------------------------------------------------------------------------------------

class _Settings(dict):
    pass


class _Encoder(object):
    def needs_graph(self):
        return True


def _toy_graph():
    # typed on purpose: relation 0 goes from entities 0..11 to 12..23, relation 1 from 12..23 to 0..11; sparse, so that
    # no pair knows every member of a list
    rng = np.random.RandomState(1)
    a = [(int(s), 0, int(o)) for s, o in zip(rng.randint(0, 12, 40), rng.randint(12, 24, 40))]
    b = [(int(s), 1, int(o)) for s, o in zip(rng.randint(12, 24, 40), rng.randint(0, 12, 40))]
    return np.array(a + b, dtype=np.int32)


@pytest.mark.parametrize("value,typed", [("Yes", True), ("No", False), (None, False)])
@pytest.mark.parametrize("exclusive", ["Yes", "No"])
def test_make_transform_host_path_honours_the_setting(value, typed, exclusive):
    from relationprediction_amd import train as train_module
    train = _toy_graph()
    settings = _Settings(NegativeSampleRate=5, EntityCount=24, RelationCount=2, GraphSplitSize=0.5,
                         ExclusiveNegativeSampling=exclusive)
    if value is not None:
        settings["TypeConstrainedNegatives"] = value
    t_func = train_module.make_transform(train, settings, _Encoder())
    K = {tuple(t) for t in train.tolist()}
    wrong_type = known_hits = 0
    for seed in range(4):
        split, X, Y = t_func.seeded(train, seed)
        n = len(train)
        assert len(X) == n * 6 and (Y[:n] == 1).all() and (Y[n:] == 0).all() and np.array_equal(X[:n], train)
        neg, src = X[n:], np.tile(train, (5, 1))
        changed = (neg != src).sum(axis=1)
        assert (changed <= 1).all() and (neg[:, 1] == src[:, 1]).all()
        if typed:
            assert (changed == 1).all()            # a typed draw is never the row's own entity
        low_subject = neg[:, 0] < 12
        low_object = neg[:, 2] < 12
        wrong_type += int((low_subject != (neg[:, 1] == 0)).sum() + (low_object != (neg[:, 1] == 1)).sum())
        known_hits += sum(tuple(t) in K for t in neg.tolist())
    assert (wrong_type == 0) == typed, wrong_type
    if exclusive == "Yes":
        assert known_hits == 0
    assert t_func.sampler.typed_open == 0            # every list of the toy graph has several members, few of them known


def test_transform_typed_is_reproducible_and_falls_open():
    from relationprediction_amd.common import auxilliaries
    train = _toy_graph()
    ns = auxilliaries.NegativeSampler(3, 24)
    ns.set_known_positives(train)
    ns.set_type_sets(np.concatenate([train, np.array([(2, 0, 7)] * 2, dtype=np.int32)]))
    a = ns.transform_typed(train[:40], np.random.RandomState(5))
    b = ns.transform_typed(train[:40], np.random.RandomState(5))
    c = ns.transform_typed(train[:40], np.random.RandomState(6))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    # a relation the sets never saw, and a singleton: drawn over all entities and counted
    ns.set_type_sets(np.array([(2, 0, 7)], dtype=np.int32))
    before = ns.typed_open
    x, _ = ns.transform_typed(train[:40], np.random.RandomState(5))
    assert ns.typed_open == before + 120 and np.array_equal(x, ns.transform(train[:40], np.random.RandomState(5))[0])


@pytest.mark.parametrize("bad", ["yes", "1", "", True])
def test_a_bad_setting_value_is_refused(bad):
    from relationprediction_amd import train as train_module
    from relationprediction_amd.common import evaluation
    settings = _Settings(NegativeSampleRate=5, EntityCount=24, GraphSplitSize=0.5, TypeConstrainedNegatives=bad)
    with pytest.raises(ValueError, match="TypeConstrainedNegatives"):
        train_module.make_transform(_toy_graph(), settings, _Encoder())
    with pytest.raises(ValueError, match="TypeConstrained"):
        evaluation.Scorer(_Settings(Metric="MRR", TypeConstrained=bad))


def test_type_constrained_evaluation_is_for_entity_ranks():
    from relationprediction_amd.common import evaluation
    for metric in ("RelationMRR", "Accuracy"):
        with pytest.raises(NotImplementedError, match="TypeConstrained"):
            evaluation.Scorer(_Settings(Metric=metric, TypeConstrained="Yes"))
        assert not evaluation.Scorer(_Settings(Metric=metric, TypeConstrained="No")).type_constrained
    assert evaluation.Scorer(_Settings(Metric="MRR", TypeConstrained="Yes")).type_constrained
    assert not evaluation.Scorer(_Settings(Metric="MRR")).type_constrained


def test_typed_scorer_asks_the_model_for_typed_ranks():
    """TypeConstrained=Yes: evaluate_mrr calls device_ranks_typed with the registered training triples, both sides; the
    default calls device_ranks as before"""
    from relationprediction_amd.common import evaluation
    train = _toy_graph()
    calls = []

    class _Model(object):
        test_graph = object()

        def device_ranks(self, graph, triples, predict_object, ptr, idx):
            calls.append(("open", predict_object))
            return np.ones(len(triples), np.int32), np.ones(len(triples), np.int32)

        def device_ranks_typed(self, graph, triples, predict_object, ptr, idx, types):
            calls.append(("typed", predict_object, types))
            return np.ones(len(triples), np.int32), np.ones(len(triples), np.int32)

    for value in ("Yes", "No"):
        scorer = evaluation.Scorer(_Settings(Metric="MRR", TypeConstrained=value))
        scorer.register_data(train)
        scorer.register_degrees(train)
        scorer.register_model(_Model())
        scorer.finalize_frequency_computation(train)
        if value == "Yes":
            with pytest.raises(ValueError, match="register_type_sets"):
                scorer.compute_scores(train[:5])
            scorer.register_type_sets(train)
        del calls[:]
        assert scorer.compute_scores(train[:5]).get_summary().results["Filtered"]["MRR"] == 1.0
        if value == "Yes":
            assert [c[:2] for c in calls] == [("typed", False), ("typed", True)]
            assert all(np.array_equal(c[2], train) for c in calls)
        else:
            assert calls == [("open", False), ("open", True)]


def test_predict_refuses_type_constrained_relation_and_ensemble_queries():
    from relationprediction_amd import predict
    base = ["--settings", "s", "--dataset", "d", "--model", "m", "--queries", "q", "--type-constrained"]
    with pytest.raises(ValueError, match="type-constrained"):
        predict.main(base + ["--side", "relation"])
    with pytest.raises(ValueError, match="type-constrained"):
        predict.main(base + ["--settings2", "s2", "--model2", "m2"])


def test_device_batches_carry_the_type_triples():
    """the device paths hand the training triples on as `types` (one array, so the runtime reserves the sets once), and
    the optimizer passes them to the model only when they are there"""
    from relationprediction_amd import train as train_module
    from relationprediction_amd.optimization.optimize import DeviceMinibatch, DeviceNegatives, HipOptimizer
    train = _toy_graph()
    for value in ("Yes", "No"):
        settings = _Settings(NegativeSampleRate=5, EntityCount=24, RelationCount=2, GraphSplitSize=0.5,
                             TypeConstrainedNegatives=value)
        a = train_module.make_transform(train, settings, _Encoder(), device_negatives=True)
        b = train_module.make_transform(train, settings, _Encoder(), device_negatives=True, device_dropout=True)
        x, y, z = a.seeded(train, 1), a.seeded(train, 2), b.seeded(train, 1)
        assert isinstance(x, DeviceNegatives) and isinstance(z, DeviceMinibatch)
        if value == "Yes":
            assert x.types is y.types is z.types and np.array_equal(x.types, train)
        else:
            assert x.types is None and z.types is None
        seen = []

        class _Model(object):
            def device_train_step_negatives(self, *args):
                seen.append(args)

        opt = HipOptimizer.__new__(HipOptimizer)
        opt.model = _Model()
        opt.update_from_batch(x, 3)
        assert len(seen[0]) == (7 if value == "Yes" else 4) and (value == "No" or seen[0][6] is x.types)
