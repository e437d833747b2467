"""Oracle of the graphlet-counting labels (test infrastructure, CPU only).

orbit_labels restates the definition of DESIGN §6d by brute force: self loops dropped, edges symmetrised, duplicates
collapsed; for each of the five patterns every subgraph monomorphism (networkx GraphMatcher: the pattern's edges must be
present, extra edges are allowed) adds 1 at [image node, orbit of the pattern node]; a copy shows up once per
automorphism of its pattern, so the sums are divided by |Aut| — exactly, which is asserted.
"""
from math import comb

import numpy as np

NUM_ORBITS = 11
# name, edges, orbit column of each pattern node, |Aut|
PATTERNS = (
    ("tailed_triangle", ((0, 1), (1, 2), (2, 0), (0, 3)), (0, 1, 1, 2), 2),
    ("chordal_cycle", ((0, 1), (1, 2), (2, 3), (3, 0), (0, 2)), (3, 4, 3, 4), 4),
    ("4_clique", ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)), (5, 5, 5, 5), 24),
    ("4_path", ((0, 1), (1, 2), (2, 3)), (6, 7, 7, 6), 2),
    ("triangle_rectangle", ((0, 1), (1, 2), (2, 0), (1, 3), (2, 4), (3, 4)), (8, 9, 9, 10, 10), 2),
)
ORBITS = ((0, 1, 2), (3, 4), (5,), (6, 7), (8, 9, 10))


def pattern_edges(name):
    """(node count, int64 [2, m] edge list, one direction) of a pattern graph"""
    for nm, edges, orbit, _ in PATTERNS:
        if nm == name:
            return len(orbit), np.array(edges, dtype=np.int64).T
    raise KeyError(name)


def clean_pairs(edge_index):
    """the kernel's normalisation: the set of undirected edges {a < b}"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    return sorted({(int(min(a, b)), int(max(a, b))) for a, b in ei.T if a != b})


def orbit_labels(n, edge_index):
    """int64 [n, 11]: for every node and orbit, the copies that hold the node at that orbit"""
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(clean_pairs(edge_index))
    out = np.zeros((n, NUM_ORBITS), dtype=np.int64)
    for _, edges, orbit, aut in PATTERNS:
        P = nx.Graph()
        P.add_edges_from(edges)
        acc = np.zeros((n, NUM_ORBITS), dtype=np.int64)
        k = len(orbit)                                                  # every mapping: graph node -> pattern node
        maps = np.array([[*m.keys(), *m.values()] for m in GraphMatcher(G, P).subgraph_monomorphisms_iter()],
                        dtype=np.int64).reshape(-1, 2 * k)
        np.add.at(acc, (maps[:, :k].ravel(), np.array(orbit)[maps[:, k:].ravel()]), 1)   # +1 per (image node, orbit)
        assert (acc % aut == 0).all()
        out += acc // aut
    return out


def orbit_sums(orbits):
    """[n, 5]: the copies of each pattern through the node, at any position"""
    o = np.asarray(orbits, dtype=np.int64)
    return np.stack([o[:, list(c)].sum(axis=1) for c in ORBITS], axis=1)


def complete_graph_edges(n):
    return np.array([(a, b) for a in range(n) for b in range(a + 1, n)], dtype=np.int64).reshape(-1, 2).T


def complete_graph_row(n):
    """the row of every node of K_n: total copies * orbit size / n"""
    totals = (3 * (n - 3) * comb(n, 3), 6 * comb(n, 4), comb(n, 4), 12 * comb(n, 4), 60 * comb(n, 5))
    sizes = (1, 2, 1, 2, 2, 4, 2, 2, 1, 2, 2)
    row = []
    for t, cols in zip(totals, ORBITS):
        for c in cols:
            assert (t * sizes[c]) % n == 0
            row.append(t * sizes[c] // n)
    return np.array(row, dtype=np.int64)


def hand_cases():
    """(name, n, int64 [2, m] edges, expected int64 [n, 11])"""
    k4 = np.array([[3, 6, 3, 3, 3, 1, 6, 6, 0, 0, 0]] * 4, dtype=np.int64)
    k5 = np.array([[12, 24, 12, 12, 12, 4, 24, 24, 12, 24, 24]] * 5, dtype=np.int64)
    house_e = np.array([(0, 1), (1, 2), (2, 0), (1, 3), (2, 4), (3, 4)], dtype=np.int64).T
    apex, shoulder, foot = [0, 2, 0, 0, 0, 0, 4, 2, 1, 0, 0], [1, 1, 0, 0, 0, 0, 3, 6, 0, 1, 0], [0, 0, 1, 0, 0, 0, 5, 3, 0, 0, 1]
    house = np.array([apex, shoulder, shoulder, foot, foot], dtype=np.int64)
    p4 = np.zeros((4, NUM_ORBITS), dtype=np.int64)
    p4[[0, 3], 6] = 1
    p4[[1, 2], 7] = 1
    return [("K4", 4, complete_graph_edges(4), k4), ("K5", 5, complete_graph_edges(5), k5),
            ("house", 5, house_e, house), ("P4", 4, pattern_edges("4_path")[1], p4)]


def messy_case():
    """(n, messy edges, cleaned edges): self loops, a duplicated edge, a one-directional edge and an isolated node (5)"""
    messy = np.array([(0, 0), (0, 1), (1, 0), (0, 1), (1, 2), (2, 1), (2, 0), (2, 3), (3, 2), (3, 3), (3, 4), (4, 3),
                      (4, 1), (1, 3)], dtype=np.int64).T
    clean = np.array([(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (1, 4), (1, 3)], dtype=np.int64).T
    return 6, messy, clean
