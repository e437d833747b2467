"""Case table of the three step engines (csrc/engine.hip: counting, ZINC, OGB) on degenerate and skewed BATCH STRUCTURE:
edge-less and one-node graphs, in-degree 0, a hub of more in-edges than a wave, E < N, the stated minimum (N >= 2, E >= 2,
G >= 2), row counts on either side of the 32- / 64-row blocks and the 4-row aggregate slots, all-identical rows.  No GPU and
no fixture file here: tests/test_engine_cases_cpu.py proves what every case claims about itself and that the CPU oracle is
well conditioned on it; tests/test_hip_engine_structure.py runs the table through the engines.

A graph is `(n, src, dst)` with int64 arrays of graph-local node ids (no RNG in the structure).  A case is a list of
graphs, one batch.  Node / edge / target data are drawn per (family, case) from a seeded torch.Generator.  The oracle batch
is built with ref_features.encode_graph (h = 2, use_rd, self loops as the family's driver sets them) and stepped once by
the family's reference model of oracle/ref_model.py in fp32 and in fp64, on ONE thread."""
import copy

import numpy as np
import torch

import ref_features as orc
import ref_model as rm

I64 = np.int64
HOPS = 2


# ---- raw graphs ------------------------------------------------------------------------------------------------------------
def _both(n, pairs):
    s = np.array([a for a, b in pairs] + [b for a, b in pairs], I64)
    t = np.array([b for a, b in pairs] + [a for a, b in pairs], I64)
    return n, s, t


def directed(n, pairs):
    return n, np.array([a for a, b in pairs], I64), np.array([b for a, b in pairs], I64)


def edgeless(n):
    return n, np.zeros(0, I64), np.zeros(0, I64)


def path(n):
    return _both(n, [(i, i + 1) for i in range(n - 1)])


def star(leaves):
    """node 0 joined to `leaves` others, both directions: in-degree `leaves` at the hub"""
    return _both(leaves + 1, [(0, i) for i in range(1, leaves + 1)])


def ring(n):
    return _both(n, [(i, (i + 1) % n) for i in range(n)])


PAIR = _both(2, [(0, 1)])
_MIXED = [path(5), edgeless(6), edgeless(1), star(40), directed(2, [(0, 1)]), edgeless(1), _both(7, [(1, 3), (3, 5)])]


def _rotated(graphs, k):
    return graphs[k:] + graphs[:k]


def _rows(n):
    return [ring(n - 2), PAIR]


# name -> the graphs of the batch.  `zero_variance` depends on whether the family adds self loops (a one-node graph has no
# edge without them), see graphs_of.
CASES = {
    "mixed": _MIXED,
    "mixed_edgeless_last": _rotated(_MIXED, 2),      # tail of in_ptr: six nodes of in-degree 0; tail of graph_ptr: no edge
    "mixed_hub_last": _rotated(_MIXED, 4),           # tail of in_ptr: the widest row
    "minimal": [PAIR, path(3)],
    "hub65": [path(3), star(65), PAIR],
    "sparse_edges": [_both(40, [(0, 1)]), directed(30, [(0, 1)])],
    "rows_64": _rows(64),
    "rows_65": _rows(65),
    "rows_129": _rows(129),
    "zero_variance": None,
}
CASE_NAMES = tuple(CASES)
# outside the table: below the engines' minimum (the refusal and the per-op hand-over)
BOUNDARY = {"single_node": [edgeless(1)], "single_path3": [path(3)]}

# what every case claims: N, G, (E, min in-degree, max in-degree) with self loops and without
CLAIMS = {
    "mixed": dict(N=63, G=7, loops=(156, 1, 41), plain=(93, 0, 40)),
    "mixed_edgeless_last": dict(N=63, G=7, loops=(156, 1, 41), plain=(93, 0, 40)),
    "mixed_hub_last": dict(N=63, G=7, loops=(156, 1, 41), plain=(93, 0, 40)),
    "minimal": dict(N=5, G=2, loops=(11, 2, 3), plain=(6, 1, 2)),
    "hub65": dict(N=71, G=3, loops=(207, 2, 66), plain=(136, 1, 65)),
    "sparse_edges": dict(N=70, G=2, loops=(73, 1, 2), plain=(3, 0, 1)),
    "rows_64": dict(N=64, G=2, loops=(190, 2, 3), plain=(126, 1, 2)),
    "rows_65": dict(N=65, G=2, loops=(193, 2, 3), plain=(128, 1, 2)),
    "rows_129": dict(N=129, G=2, loops=(385, 2, 3), plain=(256, 1, 2)),
    "zero_variance": dict(loops=dict(N=2, G=2, E=2, deg=(1, 1)), plain=dict(N=4, G=2, E=4, deg=(1, 1))),
}

# ---- families ----------------------------------------------------------------------------------------------------------------
SELF_LOOP = {"count": True, "zinc": False, "ogb": True}          # run_graphcount / run_zinc / run_ogb_mol
# (family, L, H): counting (3, 64) is the smallest shape on which every live fusion runs; (1, 32) has no hidden GINE layer, no
# batched edge GEMM and H > 32 false; ZINC has its fixed width of 256
MODELS = (("count", 3, 64), ("count", 1, 32), ("zinc", 2, 256), ("ogb", 2, 32))
# (family, L, H, case): depths around the 48 weight-gradient reduces that one launch takes (csrc/engine_plan.h: 3L+6, 3L+3 and 5L
# of them).  count 14 is the last depth whose reduces are deferred to the end of the step, the others reduce every weight gradient
# at once; each on the ONE case named — not crossed with the table: the neighbours are not conditioned (count 15/32 `mixed` 7.6e-3,
# zinc 16 `rows_64` 1.4e-2 against the cap below; tests/test_engine_cases_cpu.py holds these four to it).
# The OGB model at depth 10 and width 32 is under the cap on seven cases of the table (`mixed` 7.7e-5) and exceeds B on the MI355X
# on every one of them, by the same figure before and after the plan header and on the per-op path as well (`mixed`: per-op grad
# convs.8.mlp.3.weight 1.80e-5 against 1.72e-5, e_ref 5.7e-6; `mixed_hub_last` 1.28 B; the G = 2 cases 6 .. 29 B in the two-row
# BatchNorms of the virtual-node MLPs): ill-conditioned for the device's summation order where e_ref sits at the floor of B.  At
# width 64 `mixed_hub_last` (worst e_ref 1.9e-4, the same on two host CPUs) is held at 0.73 B on both schedules.  Not a G = 2 case:
# 10/64 `sparse_edges` is 8.8e-5 on one host CPU and 5.2e-2 on another (eval_pred, through the two-row BatchNorms' running variance).
DEEP = (("count", 14, 64, "mixed"), ("count", 15, 64, "mixed_hub_last"), ("zinc", 16, 256, "rows_65"), ("ogb", 10, 64, "mixed_hub_last"))
ZINC_NODE_TYPES, ZINC_EDGE_TYPES = 28, 4
CAP = 1e-3                                                       # conditioning cap on the fp32 oracle's own error
# Data seed of a (family, case) when it is not the default one: where the fp32 oracle exceeded the cap with the default seed.
#   count rows_64: one pre-activation within fp32 rounding of a ReLU kink (relative Frobenius error 9e-3 in conv1's gradients)
#   zinc rows_*:   G = 2, so bn_lin1 normalises TWO rows: its output is +-gamma + beta whatever comes in, the gradient below
#                  it lives on the few columns whose two rows nearly coincide (amplified by up to eps^-1/2 = 316), and how much
#                  of it there is depends on the signs of pred - y.  Of the seeds 1..79, 20 / 20 / 5 keep the oracle under 3e-4
#                  (and do so under a 1e-6 relative jitter of the weights); the default one gave 1.3e-3 / 4.8e-3 / 9.5e-3.
# And one whose oracle is under the cap but whose e_ref is a coin toss at the floor of the bound:
#   ogb rows_129:  G = 2 again, in the virtual-node MLP.  The bias of the Linear in front of its two-row BatchNorm has a gradient
#                  that is mathematically zero; what fp32 leaves of it with the default seed is 1.1e-5 on one host CPU and 2e-7
#                  on another (the two rows of d(loss)/d(out) are +-0.0833 and differ in the 4th digit), i.e. on either side of
#                  the bound's floor of 1e-5 whatever the device does.  Of the seeds 1..39, 24 is the one on which every such
#                  zero gradient stays under 1.5e-6 and everything else under 5e-5, with and without the weight jitter.
#   ogb sparse_edges: the same two-row BatchNorm; 8.6e-5 with the default seed (2.4e-4 on another host CPU), the largest of the
#                  OGB table; 11 is the first seed after the trivial ones (both rows on the same side of their targets, where
#                  nothing flows through that BatchNorm at all) that meets the criterion above.
# A ReLU-kink flip on the device would move a case here too.
DATA_SEED = {("count", "rows_64"): 1, ("zinc", "rows_64"): 31, ("zinc", "rows_65"): 36, ("zinc", "rows_129"): 21,
             ("ogb", "rows_129"): 24, ("ogb", "sparse_edges"): 11}


def model_id(model):
    return "%s_L%d_H%d" % model


def graphs_of(family, case):
    table = dict(CASES, **BOUNDARY)
    if case == "zero_variance":
        return [edgeless(1), edgeless(1)] if SELF_LOOP[family] else [PAIR, PAIR]
    return table[case]


def _seed(family, case):
    names = list(CASES) + list(BOUNDARY)
    return DATA_SEED.get((family, case), 7919 * (1 + ("count", "zinc", "ogb").index(family)) + names.index(case))


def raw_graphs(family, case):
    """per graph: dict(num_nodes, edge_index int64 [2, m], x, y and, for the molecule families, edge_attr of the INPUT edges) —
    what the product path wraps into its Data objects and the oracle batch below is built from"""
    gen = torch.Generator().manual_seed(_seed(family, case))
    out = []
    for n, s, t in graphs_of(family, case):
        m = int(s.shape[0])
        d = dict(num_nodes=n, edge_index=torch.tensor(np.stack([s, t])))
        if family == "count":
            d["x"] = torch.randn(n, 10, generator=gen)
            d["y"] = torch.randn(n, generator=gen)
        elif family == "zinc":
            d["x"] = torch.randint(0, ZINC_NODE_TYPES, (n,), generator=gen)
            d["edge_attr"] = torch.randint(0, ZINC_EDGE_TYPES, (m,), generator=gen)
            d["y"] = torch.randn(1, generator=gen)
        else:
            d["x"] = torch.stack([torch.randint(0, k, (n,), generator=gen) for k in rm.ATOM_FEATURE_DIMS], dim=1)
            d["edge_attr"] = torch.stack([torch.randint(0, k, (m,), generator=gen) for k in rm.BOND_FEATURE_DIMS],
                                         dim=1).reshape(m, 3)
            d["y"] = torch.randint(0, 2, (1, 1), generator=gen).float()
        out.append(d)
    if case == "zero_variance":                   # every row of every BatchNorm input identical: one node / edge datum for all
        first = out[0]
        for d in out:
            d["x"] = first["x"][:1].expand_as(first["x"]).clone()
            if "edge_attr" in d:
                d["edge_attr"] = first["edge_attr"][:1].expand_as(first["edge_attr"]).clone()
    return out


_ENC = {}


def _encode(n, s, t, self_loop):
    key = (n, s.tobytes(), t.tobytes(), self_loop)
    if key not in _ENC:
        _ENC[key] = orc.encode_graph(s, t, n, HOPS, True, self_loop)
    return _ENC[key]


_BATCH = {}


def oracle_batch(family, case):
    """the collated batch on the CPU (do not modify the returned tensors): x, edge_index, pos_enc, pos_index, pos_batch,
    batch, y and, for the molecule families, edge_attr (self loops filled with 1, as create_subgraphs does)"""
    if (family, case) in _BATCH:
        return _BATCH[(family, case)]
    sl = SELF_LOOP[family]
    cols = {k: [] for k in ("x", "y", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
    n0 = e0 = 0
    for g, ((n, s, t), d) in enumerate(zip(graphs_of(family, case), raw_graphs(family, case))):
        w = _encode(n, s, t, sl)
        ei = torch.tensor(np.stack([w["edge_src"], w["edge_dst"]]))
        e = int(ei.size(1))
        if "edge_attr" in d:
            ea = d["edge_attr"]
            if sl:
                ea = torch.cat([ea[torch.tensor(w["kept"], dtype=torch.bool)], ea.new_ones((n,) + tuple(ea.shape[1:]))])
            assert ea.size(0) == e
            cols["edge_attr"].append(ea)
        cols["x"].append(d["x"])
        cols["y"].append(d["y"])
        cols["edge_index"].append(ei + n0)
        cols["pos_enc"].append(torch.tensor(w["pos_enc"]))
        cols["pos_index"].append(torch.tensor(w["pos_index"]))
        cols["pos_batch"].append(torch.tensor(w["pos_batch"]) + e0)
        cols["batch"].append(torch.full((n,), g, dtype=torch.int64))
        n0, e0 = n0 + n, e0 + e
    b = {k: torch.cat(v, dim=1 if k == "edge_index" else 0) for k, v in cols.items() if v}
    b["num_graphs"] = len(cols["x"])
    _BATCH[(family, case)] = b
    return b


# ---- the oracle step -----------------------------------------------------------------------------------------------------------
def reference_model(family, L, H, seed=None):
    """the family's reference model with seeded weights, the 1-d non-bias parameters (BatchNorm weights, eps) perturbed by
    0.1 * randn as tests/test_hip_fullsize.py does"""
    torch.manual_seed(100 * L + H if seed is None else seed)
    if family == "count":
        ref = rm.NestedGINEffRef(L, H)
    elif family == "zinc":
        assert H == 256
        ref = rm.NestedGINEffZincRef(L)
    else:
        ref = rm.GNNEffRef(1, L, H, virtual_node=True, residual=True, drop_ratio=0.0, JK="last", graph_pooling="mean")
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1 and "bias" not in n:
                p.add_(0.1 * torch.randn_like(p))
    return ref


def _forward(family, model, b, double):
    fl = (lambda t: t.double()) if double else (lambda t: t)
    if family == "count":
        return model(fl(b["x"]), b["edge_index"], b["pos_enc"], b["pos_index"], b["pos_batch"], b["batch"])
    if family == "zinc":
        return model(b["x"], b["edge_index"], b["edge_attr"], b["pos_enc"], b["pos_index"], b["pos_batch"], b["batch"])
    return model(b["x"], b["edge_index"], b["edge_attr"], b["batch"], b["pos_enc"], b["pos_index"], b["pos_batch"])


def _loss(family, pred, y):
    y = y.to(pred.dtype)
    if family == "ogb":
        return torch.nn.functional.binary_cross_entropy_with_logits(pred, y.view(-1, 1))
    return torch.nn.functional.l1_loss(pred, y.view(-1, 1))


def _one_precision(family, model, b, double, train):
    out = {}
    if train:
        model.train()
        model.zero_grad()
        pred = _forward(family, model, b, double)
        loss = _loss(family, pred, b["y"])
        loss.backward()
        out.update(pred=pred.detach().clone(), loss=loss.detach().clone(),
                   grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                   buffers={n: t.detach().clone() for n, t in model.named_buffers()})
    model.eval()
    with torch.no_grad():
        out["eval_pred"] = _forward(family, model, b, double).clone()
    return out


_STEP = {}


def oracle_step(family, case, L, H, train=True):
    """dict(state: the initial fp32 state_dict, batch, fp32, fp64); each precision holds pred, loss, grads and buffers after ONE
    training step and eval_pred, the eval-mode predictions taken afterwards.  `train=False` (a batch the reference cannot
    train on): eval_pred from the initial state only.  Computed once per argument tuple; do not modify the result."""
    key = (family, case, L, H, train)
    if key in _STEP:
        return _STEP[key]
    b = oracle_batch(family, case)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # the fp32 oracle's own error sets the bound, and it moves with the reduction split
    try:
        ref = reference_model(family, L, H)
        state = {k: v.detach().clone() for k, v in ref.state_dict().items()}
        ref64 = copy.deepcopy(ref).double()
        res = dict(state=state, batch=b, fp32=_one_precision(family, ref, b, False, train),
                   fp64=_one_precision(family, ref64, b, True, train))
    finally:
        torch.set_num_threads(threads)
    _STEP[key] = res
    return res


# ---- the error measure and the bound ----------------------------------------------------------------------------------------
def error(value, truth):
    """largest absolute difference to the fp64 value over max(1, largest |fp64 value|)"""
    truth = truth.detach().double().cpu()
    diff = (value.detach().double().cpu().reshape(truth.shape) - truth).abs()
    return float(diff.max()) / max(1.0, float(truth.abs().max())) if truth.numel() else 0.0


def float_items(side):
    """(name, tensor) of everything a precision of oracle_step holds that is a floating-point tensor"""
    for k in ("pred", "loss", "eval_pred"):
        if k in side:
            yield k, side[k]
    for n, t in side.get("grads", {}).items():
        yield "grad:" + n, t
    for n, t in side.get("buffers", {}).items():
        if t.is_floating_point():
            yield "buf:" + n, t


def reference_errors(step):
    """name -> e_ref, the fp32 oracle's own error against the fp64 oracle"""
    truth = dict(float_items(step["fp64"]))
    return {n: error(t, truth[n]) for n, t in float_items(step["fp32"])}


def bound(e_ref):
    """B: as accurate as fp32 arithmetic itself on that input (criterion and margin of test_hip_fullsize._grads_vs_fp64)"""
    return max(1e-5, 3.0 * e_ref)
