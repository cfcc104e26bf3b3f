"""A host mirror of ONE draw of the device neighbourhood sampler (csrc/neighborhood.hip), numpy only, float64.

The batch is a function of (graph, seed, k) alone, so it can be predicted: the counter hash and the vertex priorities are
integer work, an Exp(1) clock is one logarithm, the host decisions of `neighborhood_sample` (component order, whole
components, boundary component, its start vertex, `want`) are restated line for line, and the pick times are a float64
Dijkstra where the device runs float32 Bellman-Ford sweeps.  What float32 can move is bounded by a DERIVED margin:

    a device pick time is a chain of at most H + 1 float32 additions of positive terms (H: the largest hop count of a
    shortest path in the tree), each within 2^-24 relative; logf is within 1 ulp (no fast-math); the float32 minimum over
    paths lies within the same bound of the float64 minimum: (H + 2) 2^-24, doubled for slack: m = (H + 4) 2^-23.

With T the `want`-th smallest pick time of the boundary component, every edge with t < T (1 - m) MUST be in the batch
and no edge with t > T (1 + m) MAY be; a draw is determined when exactly k edges may be in it -- then the batch is known
to the edge.  tests/test_nbr_grid.py holds the constants below to the source text."""
import heapq

import numpy as np

MIX_GOLDEN, MIX_OFFSET = 0x9E3779B97F4A7C15, 0x632BE5AB
MIX_MUL1, MIX_MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
PRIORITY_XOR, PRIORITY_MASK = 0x5bf03635aa2e1d47, 0xFFFFFFFFFF000000
CLOCK_SHIFT = 40                      # the top 24 bits of the hash
K_SEGMENT = 256                       # adjacency entries per wavefront
SWEEP_STEPS = (24, 32)                # launches [0,24): 1 sweep each, [24,32): 2, from 32 on: 4
K_COMPACT_BLOCK = 1024
U64 = np.uint64


def mix64(seed, idx):
    """mix64(seed, idx) of neighborhood.hip for an array of indices, in uint64 with wrapping arithmetic"""
    idx = np.atleast_1d(np.asarray(idx)).astype(U64)
    seed = np.full(1, int(seed) & (2 ** 64 - 1), dtype=U64)
    z = seed + U64(MIX_GOLDEN) * (idx + U64(MIX_OFFSET))
    z = (z ^ (z >> U64(30))) * U64(MIX_MUL1)
    z = (z ^ (z >> U64(27))) * U64(MIX_MUL2)
    return z ^ (z >> U64(31))


def vertex_priority(seed, v):
    v = np.atleast_1d(np.asarray(v)).astype(U64)
    return (mix64((int(seed) & (2 ** 64 - 1)) ^ PRIORITY_XOR, v) & U64(PRIORITY_MASK)) | v


def end_clock(seed, end):
    """Exp(1) clock of edge ends (2e: the subject's end of edge e, 2e + 1: the object's): the argument of the logarithm
    is rounded as the device rounds it, the logarithm itself is float64"""
    r = (mix64(seed, end) >> U64(CLOCK_SHIFT)).astype(np.uint32)
    x = (r.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert x.dtype == np.float32
    return -np.log(x.astype(np.float64))


def sweeps_of_launch(it):
    return 1 if it < SWEEP_STEPS[0] else (2 if it < SWEEP_STEPS[1] else 4)


def launch_of_hop(h):
    """the launch in which hop h (1-based) of a shortest path settles when every SWEEP carries it one hop on"""
    it, done = 0, 0
    while True:
        done += sweeps_of_launch(it)
        if done >= h:
            return it
        it += 1


def segments(entries):
    """wavefronts that relax a vertex with `entries` adjacency entries, as neighborhood_reserve cuts its list"""
    return (entries + K_SEGMENT - 1) // K_SEGMENT


class Graph:
    """What rgcn_neighborhood_reserve keeps of the graph: components (union-find over non-loop edges; a vertex with
    self loops only is a component of its own), edges per component, and the adjacency of non-loop edges in edge order."""

    def __init__(self, triples, V):
        t = np.asarray(triples).reshape(-1, 3)
        self.triples, self.V, self.n = t, int(V), len(t)
        s, o = t[:, 0].astype(np.int64), t[:, 2].astype(np.int64)
        self.s, self.o = s, o
        parent = list(range(self.V))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for a, b in zip(s.tolist(), o.tolist()):
            if a != b:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
        has = np.zeros(self.V, dtype=bool)
        has[s] = has[o] = True
        self.vertices = np.flatnonzero(has)                       # vertices with edges
        roots = np.array([find(v) for v in self.vertices.tolist()], dtype=np.int64)
        uniq, label = np.unique(roots, return_inverse=True)
        self.ncomp = len(uniq)
        self.comp = np.full(self.V, -1, dtype=np.int64)
        self.comp[self.vertices] = label
        self.edge_comp = self.comp[s]
        self.comp_edges = np.bincount(self.edge_comp, minlength=self.ncomp)
        order = np.argsort(self.edge_comp, kind="stable")
        cuts = np.concatenate([[0], np.cumsum(self.comp_edges)])
        self.edges_of = [order[cuts[c]:cuts[c + 1]] for c in range(self.ncomp)]
        # adjacency CSR of the non-loop edges, entries in edge order: (other vertex, the edge END at the other vertex)
        nl = np.flatnonzero(s != o)
        v = np.stack([s[nl], o[nl]], 1).ravel()
        other = np.stack([o[nl], s[nl]], 1).ravel()
        end = np.stack([2 * nl + 1, 2 * nl], 1).ravel()
        by_v = np.argsort(v, kind="stable")
        self.adj_other, self.adj_end = other[by_v], end[by_v]
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(v, minlength=self.V))])
        self.entries = np.diff(self.ptr)
        self.nseg = int(sum(segments(int(x)) for x in self.entries))
        self._seeds, self._times = {}, {}

    # ---- per seed: the host's decisions
    def seed_state(self, seed):
        """(least priority per component, its vertex, components in visiting order)"""
        if seed not in self._seeds:
            if len(self._seeds) > 64:
                self._seeds.clear()
                self._times.clear()
            p = vertex_priority(seed, self.vertices)
            c = self.comp[self.vertices]
            by = np.lexsort((p, c))                                # per component, its vertices by priority
            first = by[np.concatenate([[0], np.cumsum(np.bincount(c, minlength=self.ncomp))[:-1]])]
            cmin, cstart = p[first], self.vertices[first]
            self._seeds[seed] = (cmin, cstart, np.argsort(cmin, kind="stable"))
        return self._seeds[seed]

    def decide(self, seed, k):
        """neighborhood_sample's host part: (whole components in visiting order, boundary component, want)"""
        cmin, cstart, order = self.seed_state(seed)
        first = int(order[0])
        if self.comp_edges[first] >= k:
            return [], first, int(k)
        want, full = int(k), []
        for c in order.tolist():
            if self.comp_edges[c] < want:
                full.append(c)
                want -= int(self.comp_edges[c])
            else:
                return full, c, want
        raise ValueError("k = %d exceeds the graph's %d edges" % (k, self.n))

    # ---- per (seed, boundary component): pick times
    def distances(self, seed, c):
        """float64 Dijkstra from component c's start vertex: {vertex: (d, hops)}"""
        start = int(self.seed_state(seed)[1][c])
        clock = end_clock(seed, np.arange(2 * self.n))
        ptr, other, end = self.ptr.tolist(), self.adj_other, self.adj_end
        dist, done, heap = {start: (0.0, 0)}, set(), [(0.0, 0, start)]
        while heap:
            d, h, u = heapq.heappop(heap)
            if u in done:
                continue
            done.add(u)
            lo, hi = ptr[u], ptr[u + 1]
            x = clock[end[lo:hi] ^ 1]                              # crossing e out of u costs the clock of u's OWN end
            for w, nd in zip(other[lo:hi].tolist(), (d + x).tolist()):
                if w not in done and (w not in dist or nd < dist[w][0]):
                    dist[w] = (nd, h + 1)
                    heapq.heappush(heap, (nd, h + 1, w))
        return dist

    def pick_times(self, seed, c):
        """(edges of component c in pick order, their pick times, H, the distances)"""
        if (seed, c) not in self._times:
            dist = self.distances(seed, c)
            e = self.edges_of[c]
            d = np.zeros(self.V)
            d[list(dist)] = [x[0] for x in dist.values()]
            t = np.minimum(d[self.s[e]] + end_clock(seed, 2 * e), d[self.o[e]] + end_clock(seed, 2 * e + 1))
            by = np.lexsort((e, t))
            H = max(x[1] for x in dist.values())
            self._times[(seed, c)] = (e[by], t[by], H, dist)
        return self._times[(seed, c)]

    def deciding_entry(self, seed, c, v):
        """position, in v's adjacency list, of the entry that realises d(v) (-1: the start vertex)"""
        dist = self.pick_times(seed, c)[3]
        if dist[v][1] == 0:
            return -1
        lo, hi = int(self.ptr[v]), int(self.ptr[v + 1])
        cand = np.array([dist[w][0] for w in self.adj_other[lo:hi].tolist()]) + end_clock(seed, self.adj_end[lo:hi])
        return int(np.argmin(cand))

    def draw(self, seed, k):
        """(must, may, info) of one draw: sorted edge-id arrays and what the coverage tests ask about"""
        full, boundary, want = self.decide(seed, k)
        e, t, H, _ = self.pick_times(seed, boundary)
        m = (H + 4) * 2.0 ** -23
        T = t[want - 1]
        whole = [self.edges_of[c] for c in full]
        must = np.sort(np.concatenate(whole + [e[:np.searchsorted(t, T * (1 - m), "left")]]))
        may = np.sort(np.concatenate(whole + [e[:np.searchsorted(t, T * (1 + m), "right")]]))
        info = {"full": full, "boundary": boundary, "want": want, "boundary_edges": int(self.comp_edges[boundary]),
                "use_state": bool(full), "H": H, "margin": m, "T": float(T), "determined": len(may) == k,
                "pick": np.sort(np.concatenate(whole + [e[:want]])), "threshold_edge": int(e[want - 1])}
        return must, may, info


def mirror(triples, V, seed, k):
    """one draw of (graph, seed, k): (must, may, info).  For many draws of one graph keep a Graph and call its draw()."""
    return Graph(triples, V).draw(seed, k)
