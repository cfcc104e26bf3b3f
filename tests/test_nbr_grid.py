"""The neighbourhood sampler's grid (tests/nbr_grid.py) and its float64 mirror (tests/nbr_reference.py), held without a GPU:
the mirror's constants are the source's, every case reaches what it is in the table for, the mirror decides nearly every
draw of every case (at most 2 % undetermined), and the mirror's process is the reference's."""
import collections
import os

import numpy as np
import pytest

import oracle
import nbr_grid as grid
import nbr_reference as ref

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc",
                      "neighborhood.hip")
UNDETERMINED_CAP = 0.02
HUBS = {"hub256": 256, "hub257": 257, "hub512": 512, "hub513": 513}


@pytest.mark.parametrize("text", [
    "uint64_t z = seed + 0x%Xull * (idx + 0x%Xull);" % (ref.MIX_GOLDEN, ref.MIX_OFFSET),
    "z = (z ^ (z >> 30)) * 0x%Xull;" % ref.MIX_MUL1,
    "z = (z ^ (z >> 27)) * 0x%Xull;" % ref.MIX_MUL2,
    "return z ^ (z >> 31);",
    "return (mix64(seed ^ 0x%xull, (uint64_t)v) & 0x%Xull) | (uint64_t)(uint32_t)v;" % (ref.PRIORITY_XOR, ref.PRIORITY_MASK),
    "const uint32_t r = (uint32_t)(mix64(seed, end) >> %d);" % ref.CLOCK_SHIFT,
    "return -logf(((float)r + 0.5f) * (1.0f / 16777216.0f));",
    "kSegment = %d;" % ref.K_SEGMENT,
    "constexpr int sweeps_of_launch(int it) { return it < %d ? 1 : (it < %d ? 2 : 4); }" % ref.SWEEP_STEPS,
    "constexpr int kCompactBlock = %d;" % ref.K_COMPACT_BLOCK,
    "for (int b0 = ptr[v]; b0 < ptr[v + 1]; b0 += kSegment) {",
    "seg_v.push_back(ptr[v + 1] - ptr[v] > kSegment ? ~v : v);",
    "if (q.comp_edges_h[first] < k) {",
    "if (q.comp_edges_h[cid] < want) {",
    "other[fill[s]] = o; endid[fill[s]++] = 2 * e + 1;",
    "other[fill[o]] = s; endid[fill[o]++] = 2 * e;",
])
def test_the_mirror_follows_the_kernel_source(text):
    """nbr_reference.py restates these lines: when one changes, the mirror has to change with it."""
    with open(SOURCE) as f:
        assert text in f.read(), "neighborhood.hip no longer holds `%s`: update tests/nbr_reference.py" % text


def test_hash_on_known_values():
    """splitmix64's finaliser: mix64(0, -0x632BE5AB) is splitmix64's first output for state 0"""
    assert int(ref.mix64(0, (1 - ref.MIX_OFFSET) % 2 ** 64)[0]) == 0xE220A8397B1DCDAF
    p = ref.vertex_priority(5, np.arange(1000))
    assert len(np.unique(p)) == 1000 and np.array_equal(p & np.uint64(0xFFFFFF), np.arange(1000, dtype=np.uint64))
    x = ref.end_clock(9, np.arange(200000))
    assert x.dtype == np.float64 and (x >= 0).all() and abs(x.mean() - 1.0) < 0.01 and abs(x.var() - 1.0) < 0.03
    assert [ref.launch_of_hop(h) for h in (1, 24, 25, 26, 27, 40, 41, 44, 45)] == [0, 23, 24, 24, 25, 31, 32, 32, 33]
    assert [ref.segments(n) for n in (0, 1, 256, 257, 512, 513)] == [0, 1, 1, 2, 2, 3]


def stats(name):
    """draws, determined draws, largest H and margin of a case, and the infos of its draws"""
    g, infos = grid.graph(name), []
    for seed, ks in grid.draws(name):
        for k in ks:
            must, may, info = g.draw(seed, k)
            assert len(must) <= k <= len(may) and np.isin(must, may).all() and np.isin(info["pick"], may).all()
            assert len(info["pick"]) == k and np.isin(must, info["pick"]).all()
            infos.append((seed, k, info))
    return g, infos


@pytest.mark.parametrize("name", sorted(grid.CASES))
def test_the_mirror_determines_nearly_every_draw(name):
    """at most 2 % of a case's draws are left open by the float32 margin, and every class of k has determined draws"""
    g, infos = stats(name)
    open_ = [(s, k) for s, k, i in infos if not i["determined"]]
    print("%s: %d draws, %d determined, largest H %d, largest margin %.3g" % (
        name, len(infos), len(infos) - len(open_), max(i["H"] for _, _, i in infos), max(i["margin"] for _, _, i in infos)))
    assert len(open_) <= UNDETERMINED_CAP * len(infos), (name, len(open_), len(infos), open_[:10])
    determined = {k for s, k, i in infos if i["determined"]}
    if grid.CASES[name][2] in ("all", "fifth", "blocks"):
        assert determined == {k for _, ks in grid.draws(name) for k in ks}, "a k with no determined draw"
    if any(i["use_state"] for _, _, i in infos):
        assert any(i["use_state"] and i["determined"] for _, _, i in infos), "no determined draw with whole components"


@pytest.mark.parametrize("name", sorted(HUBS))
def test_hub_cases_reach_their_segments(name):
    g, N = grid.graph(name), HUBS[name]
    assert g.entries[grid.HUB] == N and (g.s == g.o).sum() == grid.HUB_LOOPS and g.n == N + grid.HUB_LOOPS + grid.HUB_OTHER
    assert g.V == 300 and g.entries[1:].max() < 64
    assert ref.segments(N) == {256: 1, 257: 2, 512: 2, 513: 3}[N] and N - (ref.segments(N) - 1) * ref.K_SEGMENT == \
        {256: 256, 257: 1, 512: 256, 513: 1}[N]
    # the entry that decides d(hub): every bridge position over the case's seeds, and one that is no bridge
    decided = {g.deciding_entry(seed, g.decide(seed, 1)[1], grid.HUB) for seed, _ in grid.draws(name)}
    bridges = set(grid.hub_bridges(N))
    assert bridges <= decided and decided - bridges - {-1}, (name, sorted(decided))
    assert g.n <= grid.ALL_KS_UP_TO or grid.CASES[name][2] == "fifth"


def test_two_hubs_relax_from_each_other():
    g = grid.graph("two_hubs")
    assert g.entries[0] == g.entries[1] == 270 and g.entries[2:].max() <= ref.K_SEGMENT
    assert ((g.s + g.o == 1) & (g.s * g.o == 0)).sum() == 40 and g.n <= grid.ALL_KS_UP_TO
    via = []
    for seed, _ in grid.draws("two_hubs"):
        c = g.decide(seed, 1)[1]
        if g.comp_edges[c] < 500:
            via.append("small component first")
            continue
        for v in (0, 1):
            j = g.deciding_entry(seed, c, v)
            if j >= 0 and g.adj_other[g.ptr[v] + j] == 1 - v:
                via.append((v, j // ref.K_SEGMENT))                # the hub, and the segment that holds the deciding entry
    # each hub is reached from the other one, through its first and through its second segment
    assert {(0, 0), (1, 0), (1, 1)} <= set(via) and {(0, 1), (1, 1)} & set(via) and "small component first" in via, via


def test_chains_reach_the_three_sweep_regimes():
    """With one hop per sweep the deepest path of a draw settles in launch launch_of_hop(H): before launch 24 on
    hub and block cases, inside [24, 32) and past 32 on chain60, past 32 on chain100 and the lollipop."""
    last = {name: [ref.launch_of_hop(g.pick_times(seed, g.decide(seed, 1)[1])[2]) for seed, _ in grid.draws(name)]
            for name in ("chain60", "chain100", "lollipop", "hub513") for g in [grid.graph(name)]}
    a, b = ref.SWEEP_STEPS
    assert any(a <= x < b for x in last["chain60"]) and any(x >= b for x in last["chain60"]), last
    assert all(x > b for x in last["chain100"]) and all(x >= b for x in last["lollipop"]), last
    assert all(x < a for x in last["hub513"]), last
    for name, L in (("chain60", 60), ("chain100", 100)):
        g = grid.graph(name)
        assert g.n == L and g.ncomp == 1 and sorted(g.entries.tolist()) == [1, 1] + [2] * (L - 1)
    g = grid.graph("lollipop")
    assert g.n == 360 and g.ncomp == 1 and g.entries[:60].tolist() == [1] + [2] * 59
    assert g.entries[60:].min() >= 3 and g.entries[60:].mean() > 10


@pytest.mark.parametrize("name,blocks", [("blocks1023", 1), ("blocks1024", 1), ("blocks1025", 2), ("blocks2049", 3)])
def test_block_cases_reach_their_blocks(name, blocks):
    g, infos = stats(name)
    assert (g.n + ref.K_COMPACT_BLOCK - 1) // ref.K_COMPACT_BLOCK == blocks and g.V == 3000
    assert g.comp_edges.max() > g.n // 2 and g.ncomp > 100                       # a large component and many small ones
    ks = {k for _, k, _ in infos}
    assert {k for k in (1, 2, 1023, 1024, 1025, g.n - 1, g.n) if k <= g.n} <= ks and len(ks) >= 30
    whole = [len(i["full"]) for _, _, i in infos]
    assert min(whole) == 0 and max(whole) >= g.ncomp - 1, (min(whole), max(whole))
    # the last block's last edge (alone in its block at n = 1025 and 2049) is in some batches and not in others
    assert {bool(i["pick"][-1] == g.n - 1) for _, _, i in infos if i["determined"]} == {False, True}


def test_components_case_sits_on_the_strict_less_than():
    g, infos = stats("components")
    assert sorted(g.comp_edges.tolist()) == list(range(1, 41)) and g.V == 1000 and g.V - 1 in g.vertices
    assert len(g.vertices) < g.V - 100                                           # isolated vertices
    loops_only = [c for c in range(g.ncomp) if (g.s[g.edges_of[c]] == g.o[g.edges_of[c]]).all()]
    assert sorted(g.comp_edges[loops_only].tolist()) == list(grid.COMPONENT_LOOPS_ONLY)
    exact = [(s, k) for s, k, i in infos if i["want"] == i["boundary_edges"]]
    assert len(exact) >= 5 * 10, "want == the boundary component's edge count"
    assert any(i["want"] == i["boundary_edges"] and i["use_state"] for _, _, i in infos)
    assert any(i["want"] == i["boundary_edges"] and not i["use_state"] for _, _, i in infos)
    assert any(i["want"] == 1 and i["use_state"] for _, _, i in infos)
    assert any(i["boundary"] in loops_only for _, _, i in infos), "a boundary component of self loops only"
    assert {len(i["full"]) for _, _, i in infos} >= {0, 1, 2, 9, 10, 19, 20, 38, 39}
    for seed, ks in grid.draws("components"):                                    # k = a prefix sum, and both neighbours
        sums = np.cumsum(g.comp_edges[g.seed_state(seed)[2]]).tolist()
        assert {sums[0], sums[0] + 1, sums[9] - 1, sums[9], sums[9] + 1, sums[-1]} <= set(ks)
        for d in (-1, 0, 1):                                                     # each side of the rule has determined draws
            assert any(i["determined"] for s, k, i in infos if s == seed and k - d in sums), (seed, d)


def test_degenerate_and_tiny_cases():
    g = grid.graph("loops_only")
    assert g.n == 20 and g.nseg == 0 and len(g.adj_other) == 0 and (g.s == g.o).all() and g.ncomp > 1
    assert [ks for _, ks in grid.draws("loops_only")] == [tuple(range(1, 21))] * 10
    g = grid.graph("one_edge")
    assert g.n == 1 and g.nseg == 2 and grid.draws("one_edge") == ((1, (1,)), (2, (1,)), (3, (1,)))
    for name, (s, o, V) in (("tiny_a", grid.TINY_A), ("tiny_b", grid.TINY_B)):
        g = grid.graph(name)
        assert np.array_equal(g.s, s) and np.array_equal(g.o, o) and g.V == V
        assert len(grid.draws(name)) == 50 and all(ks == tuple(range(1, g.n + 1)) for _, ks in grid.draws(name))
    _, infos = stats("tiny_a")                                                   # restarts; want == component size
    assert any(i["use_state"] for _, _, i in infos) and any(i["want"] == i["boundary_edges"] for _, _, i in infos)


def test_wide_ids_thresholds_have_bit_16():
    g, infos = stats("wide_ids")
    assert g.n == 66000 and g.V == 20000 and len(infos) == 24
    assert all(i["threshold_edge"] >= grid.WIDE_HIGH_ID and i["determined"] and not i["use_state"] for _, _, i in infos)
    ks = sorted(k for _, k, _ in infos)
    assert ks[0] < 6000 and ks[-1] > 60000


@pytest.mark.parametrize("name,ks", [("tiny_a", (3, 6)), ("tiny_b", (2, 3))])
def test_the_mirror_is_the_reference_process(name, ks):
    """Outcome sets of the mirror over 6,000 seeds against 6,000 runs of the reference's loop
    (oracle.sample_edge_neighborhood), each frequency within 4.5 standard errors: tests/test_gpu_sampler.py's bar for
    the device, here for the mirror that the device is then held to draw by draw."""
    g, n = grid.graph(name), 6000
    for k in ks:
        mir, orc = collections.Counter(), collections.Counter()
        for seed in range(n):
            mir[tuple(g.draw(20000 + seed, k)[2]["pick"].tolist())] += 1
        rng = np.random.RandomState(100 * len(name) + k)
        for _ in range(n):
            orc[tuple(sorted(oracle.sample_edge_neighborhood(g.triples, g.V, k, rng).tolist()))] += 1
        for s in set(mir) | set(orc):
            pa, pb = mir[s] / n, orc[s] / n
            p = max((pa + pb) / 2, 1e-3)
            se = np.sqrt(2 * p * (1 - min(p, 0.999)) / n)
            assert abs(pa - pb) <= 4.5 * se, (name, k, s, pa, pb)
