"""tests/pmc_exact_np.py -- restatement of the EXACT mode of the max-clique inlier selection (RSX_ORORA_PMC_EXACT,
pmc_exact_kernel in csrc/pmc.hip) in numpy + plain Python.  TEST INFRASTRUCTURE ONLY; no dependency on oracle/.

For ONE pair it takes what oracle/pmc_np.py defines -- the adjacency (K x K, symmetric, no self loops), the core numbers and
the greedy clique (member flags) -- and returns (member bool[K], size, flags, nodes).

WHAT IS RETURNED
  size   the clique number omega of the graph (unless the node budget ran out)
  which  if the greedy clique already has omega vertices: the greedy clique, unchanged.  Otherwise THE maximum clique whose
         members' ranks, sorted ascending, are the lexicographically smallest sequence; rank = position in the priority order
         (core number descending, index ascending).  Neither the traversal nor the bound enters this definition.
  flags  MAXIMUM (8) when the search completed or a bound proved the greedy clique (PROVEN (1) stays as the greedy stage set it);
         BUDGET (16) when the node budget ran out: the pair keeps its GREEDY clique, never a partial improvement.

HOW (the kernel does the same steps and counts the same nodes)
  g = |greedy|.  If g == max core + 1: proven, nothing to do (0 nodes).
  1. R = the vertices of core number >= g, in rank order: every clique of more than g vertices lies inside R (each of its
     members has >= g neighbours in it).  |R| <= g: the greedy clique is a maximum one.  (R is the g-core: every vertex already
     has >= g neighbours INSIDE R, a second peeling would remove nothing.)
  2. U = the vertices of R adjacent to all others of R: every maximum clique of R holds them.  S = R \\ U in rank order, n = |S|,
     the residual problem: a clique of S of more than need = g - |U| vertices.  (One pass is enough: a vertex adjacent to all
     of S is adjacent to all of U as well, so it already was in U.)  For equal-sized sets "lexicographically smaller sorted
     sequence" is decided by the smallest element of the symmetric difference, so the canonical clique of the graph is U plus
     the canonical clique of S.
  3. Greedy sequential colouring of S (vertices in rank order, each colour class filled in rank order): colours <= need proves
     the greedy clique at the root (0 nodes).
  4. Depth-first search over S, branching in RANK ORDER, accepting only STRICTLY larger cliques, with an explicit stack.
     A NODE is one branching vertex taken off a candidate set (one turn of the search loop that extends the clique in hand);
     each node costs at most one colouring.  best starts at max(need, 0) (need < 0: U alone beats the greedy clique).  At depth d with candidate set P (only vertices later in
     rank than the last member, restricted to core >= |U| + best):
         P empty or d + |P| <= best                       -> back up
         nodes == budget                                   -> BUDGET: greedy clique returned
         v = first of P; P -= v; C[d] = v; nodes += 1
         d + 1 > best                                      -> best = d + 1, the clique in hand is recorded
         P' = P & N(v) (restricted to core >= |U| + best)
         P' empty, d + 1 + |P'| <= best or d + 1 + colours(P') <= best -> next v
         else descend with P'
     Visiting cliques in lexicographic order of their rank sequences and keeping only strictly larger ones ends with the
     lexicographically smallest clique of size omega; every bound above only cuts subtrees that hold no clique larger than
     `best`, and the canonical clique is met while best < omega, so no valid bound can cut it."""
import numpy as np

PROVEN, PASSTHROUGH, NO_WORKSPACE, MAXIMUM, BUDGET = 1, 2, 4, 8, 16
DEFAULT_BUDGET = 1 << 18  # rsx_orora_clique_node_budget() of a new handle (how it was chosen)


def rank_order(core):
    return sorted(range(len(core)), key=lambda v: (-int(core[v]), v))


def _colours(rows, q, limit):
    """greedy sequential colouring of the vertex set q (a Python int bitset over S); stops once more than `limit` colours are
    needed (the caller only asks whether colours <= limit)"""
    k = 0
    while q:
        k += 1
        if k > limit:
            return k
        c = q
        while c:
            low = c & -c
            v = low.bit_length() - 1
            c &= ~rows[v] & ~low
            q &= ~low
    return k


def reduce(adj, core, greedy_member):
    """-> (g, R, U, S): the reduction steps 1 and 2 (lists of vertices in rank order)"""
    adj = np.asarray(adj).astype(bool)
    core = np.asarray(core)
    g = int(np.count_nonzero(greedy_member))
    R = [v for v in rank_order(core) if core[v] >= g]
    if not R:
        return g, R, [], []
    sub = adj[np.ix_(R, R)]
    uni = sub.sum(axis=1) == len(R) - 1
    return g, R, [v for v, u in zip(R, uni) if u], [v for v, u in zip(R, uni) if not u]


def exact(adj, core, greedy_member, budget=DEFAULT_BUDGET):
    """-> (member bool[K], size, flags, nodes)"""
    adj = np.asarray(adj).astype(bool)
    core = np.asarray(core).astype(np.int64)
    greedy = np.asarray(greedy_member).astype(bool)
    K = len(adj)
    g = int(greedy.sum())
    max_core = int(core.max()) if K else 0
    if g == max_core + 1:
        return greedy.copy(), g, PROVEN | MAXIMUM, 0
    g, R, U, S = reduce(adj, core, greedy)
    if len(R) <= g:
        return greedy.copy(), g, MAXIMUM, 0
    u, n = len(U), len(S)
    need = g - u
    pos = {v: i for i, v in enumerate(S)}
    rows = [0] * n
    for i, v in enumerate(S):
        for w in np.flatnonzero(adj[v]):
            j = pos.get(int(w))
            if j is not None:
                rows[i] |= 1 << j
    score = [int(core[v]) for v in S]

    def alive_mask(best):  # S is in rank order: the vertices of core >= u + best are a prefix
        return (1 << sum(1 for c in score if c >= u + best)) - 1

    def done(best, best_set, nodes):
        if best > need:  # (need < 0: U alone is larger than the greedy clique, the empty clique of S improves on it)
            member = np.zeros(K, dtype=bool)
            member[U] = True
            member[[S[i] for i in best_set]] = True
            return member, u + best, MAXIMUM | (PROVEN if u + best == max_core + 1 else 0), nodes
        return greedy.copy(), g, MAXIMUM, nodes

    best, best_set, nodes = max(need, 0), [], 0
    alive = alive_mask(best)
    if n == 0 or _colours(rows, alive, best) <= best:
        return done(best, best_set, nodes)
    P = [alive]
    C = []
    d = 0
    while True:
        Pd = P[d] & alive
        if Pd == 0 or d + bin(Pd).count("1") <= best:
            if d == 0:
                break
            d -= 1
            continue
        if nodes >= budget:
            return greedy.copy(), g, BUDGET, nodes
        nodes += 1
        low = Pd & -Pd
        v = low.bit_length() - 1
        P[d] = Pd & ~low
        del C[d:]
        C.append(v)
        if d + 1 > best:
            best, best_set = d + 1, list(C)
            alive = alive_mask(best)
        Pn = P[d] & rows[v] & alive
        if Pn == 0 or d + 1 + bin(Pn).count("1") <= best:
            continue
        if d + 1 + _colours(rows, Pn, best - d - 1) <= best:
            continue
        d += 1
        del P[d:]
        P.append(Pn)
    return done(best, best_set, nodes)


def exact_batch(po, src, dst, offsets, tau, budget=DEFAULT_BUDGET):
    """The restatement over a batch.  `po` supplies what oracle/pmc_np.py defines, by any implementation of it:
    po.pmc_adjacency(src, dst, tau), po.pmc_core_numbers(adj), po.pmc_select_batch(src, dst, offsets, tau) (the greedy stage).
    -> (member uint8[M], info like the greedy stage's with size / flags of the exact mode, nodes int64[n_pairs])"""
    member, info = po.pmc_select_batch(src, dst, offsets, tau)
    member, info = member.copy(), info.copy()
    nodes = np.zeros(len(offsets) - 1, dtype=np.int64)
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        if info["flags"][i] & PASSTHROUGH:
            continue
        adj = po.pmc_adjacency(src[a:b], dst[a:b], tau)
        m, size, flags, nodes[i] = exact(adj, po.pmc_core_numbers(adj), member[a:b], budget)
        member[a:b] = m
        info["size"][i], info["flags"][i] = size, flags
    return member, info, nodes
