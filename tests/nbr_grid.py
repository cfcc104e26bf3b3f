"""The cases of the neighbourhood sampler's grid: the smallest graphs at which each path of csrc/neighborhood.hip exists.
Every row of every graph is unique (parallel edges get different relation ids; the sampler ignores the relation), so a
drawn row maps to one edge id.  tests/test_nbr_grid.py (no GPU) holds every case to what it claims to reach and to the
cap on undetermined draws; tests/test_gpu_nbr_grid.py holds the device to tests/nbr_reference.py on every draw."""
import functools

import numpy as np

import nbr_reference as ref

HUB, HUB_LOOPS, HUB_OTHER, HUB_V = 0, 5, 300, 300
ALL_KS_UP_TO = 600                     # graphs of at most this many edges draw every k: the device's whole pick order
WIDE_HIGH_ID = 1 << 16


def unique_rows(s, o):
    """[n,3] int32 rows (s, r, o) with r = how often (s, o) occurred before"""
    seen, r = {}, []
    for a, b in zip(np.asarray(s).tolist(), np.asarray(o).tolist()):
        r.append(seen.get((a, b), 0))
        seen[(a, b)] = r[-1] + 1
    return np.stack([s, r, o], 1).astype(np.int32)


def _merge(rng, kept, rest):
    """both lists of (s, o) pairs in one edge order: `kept` keeps its relative order, `rest` fills the other places"""
    n = len(kept) + len(rest)
    at = np.zeros(n, dtype=bool)
    at[rng.choice(n, len(kept), replace=False)] = True
    out = np.zeros((n, 2), dtype=np.int64)
    out[at], out[~at] = np.asarray(kept).reshape(-1, 2), np.asarray(rest).reshape(-1, 2)
    return out


def _flip(rng, pairs):
    pairs = np.asarray(pairs).reshape(-1, 2)
    f = rng.rand(len(pairs)) < 0.5
    return np.where(f[:, None], pairs[:, ::-1], pairs)


def hub_bridges(N):
    """positions in the hub's adjacency list that lead to the rest of the graph: the ends of the 256-entry segments"""
    return sorted({0, ref.K_SEGMENT - 1, ref.K_SEGMENT, N - 1} & set(range(N)))


def hub_graph(N):
    """Vertex 0 with exactly N non-loop adjacency entries and 5 self loops.  Entries at hub_bridges(N) lead to vertices
    1..4 of a 149-vertex random part (300 edges), all others to leaves 150..299 that have no other neighbour: when the
    draw starts in the random part the hub is reached through one of the bridges, so the first and the last entry of a
    segment decide d(hub) on their own."""
    rng = np.random.RandomState(1000 + N)
    bridges = hub_bridges(N)
    hub = [(HUB, 1 + bridges.index(j)) if j in bridges else (HUB, rng.randint(150, HUB_V)) for j in range(N)]
    rest = []
    while len(rest) < HUB_OTHER:
        a, b = rng.randint(1, 150, 2)
        if a != b:
            rest.append((a, b))
    rest += [(HUB, HUB)] * HUB_LOOPS
    so = _merge(rng, _flip(rng, hub), rest)
    return unique_rows(so[:, 0], so[:, 1]), HUB_V


def two_hubs_graph():
    """hubs 0 and 1 with 270 entries each (segments of 256 + 14): 40 parallel edges between them, 230 to leaves of
    their own, and a 98-vertex random part of 80 edges that hangs on hub 0 by two of those entries"""
    rng = np.random.RandomState(77)
    a = [(0, 1)] * 40 + [(0, 2), (0, 3)] + [(0, rng.randint(100, 200)) for _ in range(228)]
    b = [(1, rng.randint(200, 300)) for _ in range(230)]
    hubs = np.asarray(a + b)[rng.permutation(len(a) + len(b))]
    rest = []
    while len(rest) < 80:
        x, y = rng.randint(2, 100, 2)
        if x != y:
            rest.append((x, y))
    so = _merge(rng, _flip(rng, hubs), rest)
    return unique_rows(so[:, 0], so[:, 1]), 300


def chain_graph(L, blob=0, blob_edges=0):
    """a chain of L edges (vertices 0..L, every edge in a random direction); with `blob`, its last vertex is one of a
    dense random part of `blob` vertices"""
    rng = np.random.RandomState(500 + L + blob)
    chain = _flip(rng, np.stack([np.arange(L), np.arange(1, L + 1)], 1))
    rest = []
    while len(rest) < blob_edges:
        x, y = rng.randint(L, L + blob, 2)
        if x != y:
            rest.append((x, y))
    so = _merge(rng, chain, _flip(rng, rest)) if rest else chain[rng.permutation(L)]
    return unique_rows(so[:, 0], so[:, 1]), L + 1 + max(blob - 1, 0)


def blocks_graph(n):
    """n random edges over 3,000 vertices, half of them among the first 400: one large component and many small ones"""
    rng = np.random.RandomState(n)
    dense = rng.rand(n) < 0.5
    s = np.where(dense, rng.randint(0, 400, n), rng.randint(0, 3000, n))
    o = np.where(dense, rng.randint(0, 400, n), rng.randint(0, 3000, n))
    return unique_rows(s, o), 3000


COMPONENT_LOOPS_ONLY = (3, 7, 19)


def components_graph():
    """40 components of 1..40 edges: c self loops on one vertex (c = 3, 7, 19), a path with one self loop (c divisible
    by 5), a cycle (other even c) or a path; vertex ids shuffled among 1,000 (some 190 vertices isolated, V - 1 is not)"""
    rng = np.random.RandomState(40)
    V, so, nv = 1000, [], 0
    for c in range(1, 41):
        if c in COMPONENT_LOOPS_ONLY:
            so += [(nv, nv)] * c
            nv += 1
        elif c % 5 == 0:
            so += [(nv + i, nv + i + 1) for i in range(c - 1)] + [(nv + c // 2, nv + c // 2)]
            nv += c
        elif c % 2 == 0:
            so += [(nv + i, nv + (i + 1) % c) for i in range(c)]
            nv += c
        else:
            so += [(nv + i, nv + i + 1) for i in range(c)]
            nv += c + 1
    ids = rng.permutation(V)[:nv]
    if V - 1 not in ids:
        ids[rng.randint(nv)] = V - 1
    so = ids[_flip(rng, so)][rng.permutation(len(so))]
    return unique_rows(so[:, 0], so[:, 1]), V


def loops_graph():
    rng = np.random.RandomState(20)
    v = rng.choice([0, 2, 3, 5, 8, 11], 20)
    return unique_rows(v, v), 12


def wide_graph():
    rng = np.random.RandomState(66)
    return unique_rows(rng.randint(0, 20000, 66000), rng.randint(0, 20000, 66000)), 20000


TINY_A = ([0, 1, 2, 2, 3, 4, 4, 5], [1, 2, 0, 3, 3, 5, 5, 6], 8)          # test_gpu_sampler.py's TINY, rows made unique
TINY_B = ([0, 1, 2, 3, 0], [1, 2, 3, 4, 2], 5)

# name -> (graph builder, seeds, ks rule); the rules are resolved by draws()
CASES = {
    "tiny_a": (lambda: (unique_rows(*TINY_A[:2]), TINY_A[2]), range(100, 150), "all"),
    "tiny_b": (lambda: (unique_rows(*TINY_B[:2]), TINY_B[2]), range(100, 150), "all"),
    "hub256": (lambda: hub_graph(256), (1, 2, 10), "all"),
    "hub257": (lambda: hub_graph(257), (1, 2, 3, 6), "all"),
    "hub512": (lambda: hub_graph(512), (1, 2, 3, 6, 17), "fifth"),
    "hub513": (lambda: hub_graph(513), (1, 2, 10, 12, 32), "fifth"),
    "two_hubs": (two_hubs_graph, (1, 15, 19, 26), "all"),
    "chain60": (lambda: chain_graph(60), range(1, 11), "all"),
    "chain100": (lambda: chain_graph(100), range(1, 11), "all"),
    "lollipop": (lambda: chain_graph(60, 40, 300), (1, 2, 3, 4), "all"),
    "blocks1023": (lambda: blocks_graph(1023), range(1, 6), "blocks"),
    "blocks1024": (lambda: blocks_graph(1024), range(1, 6), "blocks"),
    "blocks1025": (lambda: blocks_graph(1025), range(1, 6), "blocks"),
    "blocks2049": (lambda: blocks_graph(2049), range(1, 6), "blocks"),
    "components": (components_graph, range(1, 11), "components"),
    "loops_only": (loops_graph, range(1, 11), "all"),
    "one_edge": (lambda: (np.array([[2, 0, 0]], dtype=np.int32), 3), (1, 2, 3), "all"),
    "wide_ids": (wide_graph, (1, 2), "wide"),
}
COMPONENT_JS = (1, 2, 3, 5, 10, 20, 30, 39, 40)


@functools.lru_cache(maxsize=None)
def graph(name):
    """the case's graph as the mirror holds it (built once, never written to)"""
    triples, V = CASES[name][0]()
    triples.setflags(write=False)
    assert len(np.unique(triples, axis=0)) == len(triples), name
    return ref.Graph(triples, V)


def relations(name):
    return int(graph(name).triples[:, 1].max()) + 1


@functools.lru_cache(maxsize=None)
def draws(name):
    """the case's draws: ((seed, (k, ...)), ...)"""
    g, (_, seeds, rule) = graph(name), CASES[name]
    n, out = g.n, []
    for seed in seeds:
        if rule == "all":
            assert n <= ALL_KS_UP_TO, name
            ks = range(1, n + 1)
        elif rule == "fifth":
            ks = sorted(set(range(1, n + 1, 5)) | {2, n - 1, n})
        elif rule == "blocks":
            rng = np.random.RandomState(10 * n + seed)
            ks = sorted({k for k in (1, 2, 1023, 1024, 1025, n - 1, n) if 1 <= k <= n}
                        | set(rng.randint(1, n + 1, 30).tolist()))
        elif rule == "components":
            # the sum of the first j components in the visiting order, and that +-1: both sides of the strict `<`
            sums = np.cumsum(g.comp_edges[g.seed_state(seed)[2]])
            ks = sorted({int(sums[j - 1]) + d for j in COMPONENT_JS for d in (-1, 0, 1)} & set(range(1, n + 1)))
        elif rule == "wide":
            # k = the pick rank of an edge with id >= 2^16, so that the select's threshold key has edge-id bit 16 set:
            # twelve of them, spread over the pick order, among the draws the mirror determines
            e, t, H, _ = g.pick_times(seed, g.decide(seed, 1)[1])
            m = (H + 4) * 2.0 ** -23
            ok = (np.searchsorted(t, t * (1 + m), "right") == np.arange(1, len(t) + 1)) & (e >= WIDE_HIGH_ID)
            ranks = np.flatnonzero(ok) + 1
            ks = sorted(set(ranks[np.linspace(0, len(ranks) - 1, 12).astype(int)].tolist()))
        out.append((seed, tuple(ks)))
    return tuple(out)
