"""Datasets for the counting benchmark.

The reference reads data/count_cycle/raw/data.mat through GraphCountDataset.py:97-120 and applies
create_subgraphs as pre_transform.  The raw .mat files are not shipped (.MISSING_LARGE_BLOBS), so the
default here is the deterministic synthetic "count_cycle shape" generator of SURVEY.md §8(d):
graph g is a random d-regular graph on n nodes, (n,d) = [(10,6),(15,6),(20,5),(30,5)][g % 4],
networkx seed g; edges in np.where(A==1) order (GraphCountDataset.py:72); x = ones[n,10] (:84);
y = per-node triangle counts.  `load_count_mat` reads a real data.mat when one is present.
"""
import numpy as np
import torch

from .data import Data
from .utils_edge_efficient import create_subgraphs_many

COUNT_SHAPE_MIX = ((10, 6), (15, 6), (20, 5), (30, 5))


def count_shape_adjacency(g):
    import networkx as nx
    n, d = COUNT_SHAPE_MIX[g % 4]
    G = nx.random_regular_graph(d, n, seed=g)
    A = np.zeros((n, n), dtype=np.float32)
    for a, b in G.edges():
        A[a, b] = A[b, a] = 1.0
    return A


def adjacency_to_data(A, y):
    """GraphCountDataset.adj2data (:69-84): edge order of np.where(A == 1), x = ones[n,10]."""
    begin, end = np.where(A == 1.0)
    n = A.shape[0]
    return Data(x=torch.ones(n, 10), edge_index=torch.tensor(np.stack([begin, end]).astype(np.int64)),
                y=torch.as_tensor(y), num_nodes=n)


COUNT_LABELS = ("triangle", "cycles", "graphlets", "graphlet_orbits")


def synthetic_count_graphs(first, count, labels="triangle"):
    """labels: "triangle" — y float32 [n], the triangles through the node (host arithmetic); "cycles" — y float32 [n, 4],
    the 3..6-cycles (cycles.cycle_counts); "graphlets" — y float32 [n, 5], the copies of the five count_graphlet patterns
    through the node; "graphlet_orbits" — y float32 [n, 11], the same per orbit (graphlets.py).  The last three are
    counted on the device.  Graphs, edge order and x do not depend on `labels`."""
    if labels not in COUNT_LABELS:
        raise ValueError("labels=%r: one of %s" % (labels, ", ".join(COUNT_LABELS)))
    out = []
    for g in range(first, first + count):
        A = count_shape_adjacency(g)
        tri = (np.diagonal(A @ A @ A) / 2.0).astype(np.float32)
        out.append(adjacency_to_data(A, tri))
    if labels == "triangle":
        return out
    if labels == "cycles":
        from .cycles import cycle_counts as count
    elif labels == "graphlets":
        from .graphlets import graphlet_counts as count
    else:
        from .graphlets import graphlet_orbit_counts_float as count
    for d, y in zip(out, count(out)):
        d.y = y
    return out


def build_count_dataset(first, count, h=3, use_rd=True, self_loop=True, labels="triangle"):
    """Synthetic graphs + ESC features (HIP feature builder), as run_graphcount.py:404-408 configures it."""
    raw = synthetic_count_graphs(first, count, labels)
    done = create_subgraphs_many(raw, h, use_rd=use_rd, self_loop=self_loop)
    for d in done:
        d.num_nodes = None            # like the reference's new Data: num_nodes is inferred from x
    return done


def load_count_mat(path, split="train", target=0):
    """Read the benchmark's data.mat (reference GraphCountDataset.process :97-111)."""
    import scipy.io as scio
    raw = scio.loadmat(path)
    idx = {"train": "train_idx", "val": "val_idx", "test": "test_idx"}[split]
    if raw["F"].shape[0] == 1:
        ids = raw[idx][0]
        pairs = [(raw["A"][0][i], raw["F"][0][i]) for i in ids]
    else:
        pairs = list(zip(raw["A"][0][raw[idx]][0], raw["F"][raw[idx]][0]))
    out = []
    for A, y in pairs:
        y = np.asarray(y)
        if y.ndim == 1:
            y = y.reshape(1, -1)
        d = adjacency_to_data(np.asarray(A, dtype=np.float32), y)
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------
# Molecule-shaped synthetic sets: ZINC.pkl and the OGB downloads are absent offline, so the ZINC /
# OGB drivers default to seeded trees-with-rings of the same size and feature layout.
# ---------------------------------------------------------------------------------------------------------
def molecule_like_edges(seed, n_lo=18, n_hi=30):
    """Random tree on n in [n_lo, n_hi] nodes + 1-3 ring-closing edges; both directions, sorted by (src, dst)."""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(n_lo, n_hi + 1))
    und = {(int(rng.randint(0, i)), i) for i in range(1, n)}
    rings = 0
    for _ in range(int(rng.randint(1, 4))):
        for _try in range(20):
            a, b = sorted(map(int, rng.randint(0, n, size=2)))
            if a != b and (a, b) not in und:
                und.add((a, b))
                rings += 1
                break
    both = sorted(und | {(b, a) for a, b in und})
    ei = np.array(both, dtype=np.int64).T
    return n, ei, rings, rng


def synthetic_zinc_graphs(first, count):
    """ZINC layout (dataset_zinc.py:56-72): x int64[n] atom type in [0,28), edge_attr int64[E] bond type in [0,4),
    y float[1] (a smooth function of the topology so that training has signal)."""
    out = []
    for g in range(first, first + count):
        n, ei, rings, rng = molecule_like_edges(1000 + g)
        x = torch.tensor(rng.randint(0, 28, size=n))
        bond = rng.randint(0, 4, size=ei.shape[1])
        key = {}
        for k in range(ei.shape[1]):                       # same bond type in both directions
            a, b = int(ei[0, k]), int(ei[1, k])
            bond[k] = key.setdefault((min(a, b), max(a, b)), bond[k])
        deg = np.bincount(ei[0], minlength=n)
        y = float(rings) + 0.25 * float((deg >= 3).sum()) + 0.05 * float(x.float().mean())
        out.append(Data(x=x, edge_index=torch.tensor(ei), edge_attr=torch.tensor(bond), y=torch.tensor([y]),
                        num_nodes=n))
    return out


def synthetic_ogbmol_graphs(first, count, num_tasks=1, nan_ratio=0.0):
    """ogbg-mol* layout: x int64[n,9] (AtomEncoder columns), edge_attr int64[E,3] (BondEncoder columns),
    y float[1,num_tasks] in {0,1} with optional NaN (unlabeled) entries as in ogbg-molpcba."""
    from .ogb_mol_gnn import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS
    out = []
    for g in range(first, first + count):
        n, ei, rings, rng = molecule_like_edges(5000 + g, 12, 40)
        x = np.stack([rng.randint(0, d, size=n) for d in ATOM_FEATURE_DIMS], axis=1)
        ea = np.stack([rng.randint(0, d, size=ei.shape[1]) for d in BOND_FEATURE_DIMS], axis=1)
        score = rings + (x[:, 0] % 7 == 0).sum() * 0.5
        y = np.array([[float((score + t) % 3 >= 1.5) for t in range(num_tasks)]], dtype=np.float32)
        if nan_ratio > 0:
            y[0, rng.rand(num_tasks) < nan_ratio] = np.nan
        out.append(Data(x=torch.tensor(x), edge_index=torch.tensor(ei), edge_attr=torch.tensor(ea), y=torch.tensor(y),
                        num_nodes=n))
    return out


def build_feature_dataset(raw, h, use_rd=True, self_loop=False):
    done = create_subgraphs_many(raw, h, use_rd=use_rd, self_loop=self_loop)
    for d in done:
        d.num_nodes = None
    return done


def _ring_closing_edges(seed, n_lo=18, n_hi=30):
    """Random tree on n in [n_lo, n_hi] nodes + 1-4 ring closures between tree nodes 2..5 apart (3- to 6-rings; a closure
    may cut across an earlier ring, giving fused ring systems); both directions, sorted by (src, dst)."""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(n_lo, n_hi + 1))
    parent = [-1] + [int(rng.randint(0, i)) for i in range(1, n)]
    und = {(parent[i], i) for i in range(1, n)}
    depth = [0] * n
    for i in range(1, n):
        depth[i] = depth[parent[i]] + 1

    def tree_dist(a, b):
        d = 0
        while a != b:
            if depth[a] < depth[b]:
                a, b = b, a
            a, d = parent[a], d + 1
        return d

    for _ in range(int(rng.randint(1, 5))):
        for _try in range(40):
            a, b = sorted(map(int, rng.randint(0, n, size=2)))
            if a != b and (a, b) not in und and 2 <= tree_dist(a, b) <= 5:
                und.add((a, b))
                break
    both = sorted(und | {(b, a) for a, b in und})
    return n, np.array(both, dtype=np.int64).T, rng


def synthetic_zinc_cycle_graphs(first, count):
    """ZINC cycle-counting layout (reference dataset_zinc_cycle.py:45-61): the ZINC node / edge fields of
    synthetic_zinc_graphs (atom type in [0,28), bond type in [0,4), coalesced edges in both directions) on seeded
    ring-closed trees, and y = float32 [n, 4]: the 3-, 4-, 5- and 6-cycles through every node, counted on the device
    (cycles.cycle_counts)."""
    from .cycles import cycle_counts
    out = []
    for g in range(first, first + count):
        n, ei, rng = _ring_closing_edges(90000 + g)
        x = torch.tensor(rng.randint(0, 28, size=n))
        bond = rng.randint(0, 4, size=ei.shape[1])
        key = {}
        for k in range(ei.shape[1]):                       # same bond type in both directions
            a, b = int(ei[0, k]), int(ei[1, k])
            bond[k] = key.setdefault((min(a, b), max(a, b)), bond[k])
        out.append(Data(x=x, edge_index=torch.tensor(ei), edge_attr=torch.tensor(bond), y=None, num_nodes=n))
    for d, y in zip(out, cycle_counts(out)):
        d.y = y
    return out


# ---------------------------------------------------------------------------------------------------------
# The expressiveness datasets (the two graph files the reference ships): SR25 and EXP.
# ---------------------------------------------------------------------------------------------------------
def _both_directions_sorted(pairs):
    """to_undirected + coalesce: every pair in both directions, duplicates removed, sorted by (src, dst)"""
    both = sorted({(int(a), int(b)) for a, b in pairs} | {(int(b), int(a)) for a, b in pairs})
    if not both:
        return torch.zeros((2, 0), dtype=torch.int64)
    return torch.tensor(both, dtype=torch.int64).t().contiguous()


def load_sr25(path):
    """data/sr25/raw/sr251256.g6 (SRDataset.py:30-39): one graph6 record per line, read with networkx;
    x = ones[n, 1], edge_index = to_undirected(edge list), y = None."""
    import networkx as nx
    graphs = nx.read_graph6(path)
    if not isinstance(graphs, list):
        graphs = [graphs]
    out = []
    for G in graphs:
        n = G.number_of_nodes()
        out.append(Data(x=torch.ones(n, 1), edge_index=_both_directions_sorted(G.edges()), y=None, num_nodes=n))
    return out


def load_exp_txt(path, limit=None):
    """data/EXP/GRAPHSAT.txt (PlanarSATPairsDataset + run_exp.py:50-53).  Line 1: the number of graphs; per graph a
    line `n label`, then n lines `node_label degree neighbour ...`.  x = one_hot(node_label, 2), y = int64 [1],
    edges in both directions sorted by (src, dst)."""
    if str(path).endswith(".pkl"):
        raise ValueError("%s: the reference's .pkl raw files hold pickled torch_geometric objects and are not supported; "
                         "pass the text file (GRAPHSAT.txt) instead" % path)
    out = []
    with open(path) as fh:
        total = int(fh.readline())
        count = total if limit is None else min(total, int(limit))
        for _ in range(count):
            n, label = (int(v) for v in fh.readline().split())
            node_label, pairs = [], []
            for i in range(n):
                parts = [int(v) for v in fh.readline().split()]
                node_label.append(parts[0])
                pairs.extend((i, nb) for nb in parts[2:2 + parts[1]])
            x = torch.nn.functional.one_hot(torch.tensor(node_label, dtype=torch.int64), num_classes=2).to(torch.float)
            out.append(Data(x=x, edge_index=_both_directions_sorted(pairs), y=torch.tensor([label], dtype=torch.int64),
                            num_nodes=n))
    return out


def build_expressive_dataset(raw, h=3):
    """the pre_transform of run_sr.py:76-78 / run_exp.py:76-78: create_subgraphs(g, h, node_label='hop', use_rd=False,
    self_loop=True) for every graph, on the HIP feature builder"""
    return build_feature_dataset(raw, h, use_rd=False, self_loop=True)


def exp_split(num_graphs, split, splits=10, modulo=4, mod_thresh=1):
    """Index lists of fold `split` of the EXP protocol (run_exp.py:282-303): test = [split*n, (split+1)*n) with
    n = num_graphs // splits, divided into `lrn` (index % modulo <= mod_thresh) and `exp` (the others); of the remaining
    graphs, in order, the split-th tenth is the validation set and the rest the training set."""
    n = num_graphs // splits
    test = list(range(split * n, (split + 1) * n))
    lrn = [i for i in test if i % modulo <= mod_thresh]
    exp = [i for i in test if i % modulo > mod_thresh]
    rest = [i for i in range(num_graphs) if not split * n <= i < (split + 1) * n]
    m = len(rest) // splits
    val = rest[split * m:(split + 1) * m]
    train = rest[:split * m] + rest[(split + 1) * m:]
    return dict(train=train, val=val, test=test, lrn=lrn, exp=exp)


# ---------------------------------------------------------------------------------------------------------
# QM9-shaped synthetic molecules (the QM9 download is absent offline): the fields run_qm9.py reads.
# ---------------------------------------------------------------------------------------------------------
QM9_ATOMIC_NUMBERS = (1, 6, 7, 8, 9)                       # node_type r <-> atomic number QM9_ATOMIC_NUMBERS[r]
_QM9_MIX = np.random.RandomState(20240).uniform(-1.0, 1.0, size=(12, 8))      # fixed target mixing (12 targets x 8 descriptors)


def _embed_molecule(n, ei, rng):
    """pos float32 [n, 3]: node 0 at the origin, every other atom 1-1.6 away from its parent in the breadth-first tree of
    the bond graph and at least 0.7 away from every atom placed before it (no two atoms coincide).  A ring-closing bond
    joins two atoms the tree placed independently, so it may be longer."""
    nbrs = [[] for _ in range(n)]
    for a, b in ei.T:
        nbrs[int(a)].append(int(b))
    pos = np.zeros((n, 3), dtype=np.float64)
    placed, order = {0}, [0]
    for u in order:
        for v in nbrs[u]:
            if v in placed:
                continue
            for _try in range(200):
                d = rng.randn(3)
                cand = pos[u] + d / np.linalg.norm(d) * rng.uniform(1.0, 1.6)
                if min(np.linalg.norm(pos[w] - cand) for w in placed) >= 0.7:
                    break
            pos[v] = cand
            placed.add(v)
            order.append(v)
    return pos.astype(np.float32)


def synthetic_qm9_graphs(first, count):
    """QM9 layout (reference run_qm9.py:198-231, qm9_models.py:106-107): x float [n, 8] (column 0 the atomic number from
    {1, 6, 7, 8, 9}, columns 1-6 binary, column 7 a small count), node_type int64 [n] in [0, 5) (the index of the atomic
    number), pos float [n, 3], edge_attr float one-hot [E, 4], coalesced edges in both directions, y float [1, 12] (smooth
    functions of composition and geometry, so that training has signal), name str.  7-29 atoms, seeded by graph id."""
    out = []
    for g in range(first, first + count):
        n, ei, rings, rng = molecule_like_edges(70000 + g, 7, 29)
        node_type = rng.choice(5, size=n, p=(0.45, 0.35, 0.08, 0.1, 0.02))
        pos = _embed_molecule(n, ei, rng)
        x = np.zeros((n, 8), dtype=np.float32)
        x[:, 0] = np.array(QM9_ATOMIC_NUMBERS)[node_type]
        x[:, 1:7] = rng.randint(0, 2, size=(n, 6))
        deg = np.bincount(ei[0], minlength=n)
        x[:, 7] = np.minimum(deg, 4)
        bond = rng.randint(0, 4, size=ei.shape[1])
        key = {}
        for k in range(ei.shape[1]):                       # same bond type in both directions
            a, b = int(ei[0, k]), int(ei[1, k])
            bond[k] = key.setdefault((min(a, b), max(a, b)), bond[k])
        edge_attr = np.zeros((ei.shape[1], 4), dtype=np.float32)
        edge_attr[np.arange(ei.shape[1]), bond] = 1.0
        centred = pos.astype(np.float64) - pos.mean(0)
        blen = np.linalg.norm(pos[ei[1]] - pos[ei[0]], axis=1).astype(np.float64)
        desc = np.array([np.sqrt((centred ** 2).sum(1).mean()), n / 10.0, float((node_type > 0).mean()), x[:, 0].sum() / 50.0,
                         blen.mean(), float(rings), float((bond == 0).mean()), x[:, 1:7].mean()])
        y = _QM9_MIX @ desc + 0.1 * np.sin(_QM9_MIX @ desc * 3.0)
        out.append(Data(x=torch.tensor(x), edge_index=torch.tensor(ei), edge_attr=torch.tensor(edge_attr),
                        y=torch.tensor(y.astype(np.float32)).view(1, 12), pos=torch.tensor(pos),
                        node_type=torch.tensor(node_type, dtype=torch.int64), name="syn_qm9_%06d" % g, num_nodes=n))
    return out


def build_qm9_dataset(raw, h=3, target=0, **distance_flags):
    """The dataset of run_qm9.py:198-231 for NestedGIN_eff: create_subgraphs(g, h, use_rd=True, self_loop=True) on the HIP
    feature builder, y = y[:, target] (MyTransform), then the Distance transform (geometry.edge_distance_many; flags norm,
    squared, relative_pos, ...) once the self loops exist — edge_attr becomes [bond one-hot | distance]."""
    from .geometry import edge_distance_many
    done = create_subgraphs_many(raw, h, use_rd=True, self_loop=True)
    for d in done:
        d.num_nodes = None
        d.y = d.y[:, int(target)]
    return edge_distance_many(done, **distance_flags)


# ---------------------------------------------------------------------------------------------------------
# CSL (circular skip links): a defined graph family, generated here instead of read from the benchmark's pickle.
# ---------------------------------------------------------------------------------------------------------
CSL_SKIPS = (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)             # class k <-> skip length CSL_SKIPS[k]


def csl_edge_index(num_nodes, skip, perm=None):
    """The cycle 0 - 1 - ... - (n-1) - 0 plus the skip links i - (i + skip) mod n, node i renamed perm[i]; both directions,
    sorted by (src, dst).  4-regular for 1 < skip < n - 1, 2 * skip != n."""
    i = np.arange(num_nodes)
    pairs = np.concatenate([np.stack([i, (i + 1) % num_nodes], 1), np.stack([i, (i + skip) % num_nodes], 1)])
    if perm is not None:
        pairs = np.asarray(perm)[pairs]
    return _both_directions_sorted(pairs.tolist())


def csl_graphs(num_nodes=41, skips=CSL_SKIPS, copies=15, seed=0):
    """The CSL classification set (reference run_csl.py:83 reads it as GNNBenchmarkDataset 'CSL'): len(skips) classes of
    `copies` isomorphic graphs each, class by class.  Copy 0 of a class keeps the cycle labelling, the others are relabelled
    by permutations drawn in order from np.random.RandomState(seed).  y = int64 [1] class index; x = ones[n, 1], which is
    what the reference model substitutes when a graph has no x (run_csl.py:205-208)."""
    rng = np.random.RandomState(seed)
    out = []
    for k, skip in enumerate(skips):
        for c in range(copies):
            perm = rng.permutation(num_nodes) if c else None
            out.append(Data(x=torch.ones(num_nodes, 1), edge_index=csl_edge_index(num_nodes, int(skip), perm),
                            y=torch.tensor([k], dtype=torch.int64), num_nodes=num_nodes))
    return out


def build_csl_dataset(graphs, h=4):
    """the pre_transform of run_csl.py:78-80: create_subgraphs(g, h, node_label='hop', use_rd=True, self_loop=True) for
    every graph, on the HIP feature builder"""
    return build_feature_dataset(graphs, h, use_rd=True, self_loop=True)


def csl_k_fold(labels, folds=10, seed=12345):
    """The split protocol of the reference's kernel/train_eval.py:225-240: stratified, shuffled test folds; the validation
    fold of split i is the test fold of split i - 1 (split 0 takes the last one); training is everything else.  Returns
    (train, test, val): three lists of `folds` sorted int64 index arrays.

    Pure numpy.  The folds have the sizes and per-class counts of scikit-learn's StratifiedKFold(folds, shuffle=True) —
    class k gives fold i as many graphs as there are k's among sorted(labels)[i::folds], placed by one shuffle per class
    from np.random.RandomState(seed) — but not necessarily its permutation: which graph lands in which fold is this
    function's own."""
    y = np.asarray(labels).reshape(-1)
    classes, y_enc = np.unique(y, return_inverse=True)
    if folds < 2 or np.bincount(y_enc).max() < folds:
        raise ValueError("csl_k_fold: %d folds need at least %d graphs in some class" % (folds, folds))
    y_sorted = np.sort(y_enc)
    alloc = np.stack([np.bincount(y_sorted[i::folds], minlength=len(classes)) for i in range(folds)])    # [fold, class]
    rng = np.random.RandomState(seed)
    fold_of = np.empty(len(y), dtype=np.int64)
    for k in range(len(classes)):
        f = np.arange(folds).repeat(alloc[:, k])
        rng.shuffle(f)
        fold_of[y_enc == k] = f
    test = [np.where(fold_of == i)[0].astype(np.int64) for i in range(folds)]
    val = [test[i - 1] for i in range(folds)]
    train = []
    for i in range(folds):
        mask = np.ones(len(y), dtype=bool)
        mask[test[i]] = False
        mask[val[i]] = False
        train.append(np.where(mask)[0].astype(np.int64))
    return train, test, val
