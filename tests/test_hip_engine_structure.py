"""The three step engines (csrc/engine.hip; StepEngine, ZincStepEngine, OgbStepEngine) on the batch structures of
tests/engine_cases.py: edge-less and one-node graphs, in-degree 0, a 65-edge hub, E < N, N / E / G at the stated minimum, row
counts around the 32- and 64-row blocks and the 4-row aggregate slots, a small batch right after a large one on the same
workspace, all-identical rows.  The kernels under the engines are tested on such structure one by one elsewhere; here it is
the engines' own decisions — workspace layout, slot and block counts, the fusions picked from the batch's shape, the one- and
two-stream schedules — that are held against the fp64 CPU oracle.

Bound B(t) of a tensor t: error against fp64 (largest |difference| over max(1, largest |fp64 value|)) at most
max(1e-5, 3 * e_ref(t)), e_ref the fp32 CPU oracle's own error for t (test_engine_cases_cpu.py caps it at 1e-3, so the relative
part cannot hide a failure).  No Frobenius / ReLU-kink allowance.  Every figure is printed with its e_ref.

The batch comes through the product path (Data list -> build_feature_dataset -> DeviceGraphStore -> collate) and is first
checked to be integer-equal to the oracle's batch."""
import copy

import pytest
import torch

from conftest import require_gpu
import engine_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHEDULES = {"one_stream": 12000, "two_streams": 0}        # esc_engine_set_two_stream_min_edges
FAMILIES = ("count", "zinc", "ogb")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


@pytest.fixture
def schedule_knobs():
    """always back to the library's defaults, whatever the test set"""
    from esc_gnn_amd import _native as nv
    yield nv
    nv.call("esc_engine_set_side_stream", 2)
    nv.call("esc_engine_set_two_stream_min_edges", 12000)


# ---- the product path ---------------------------------------------------------------------------------------------------------
_STORES = {}


def device_batch(E, family, case):
    """a fresh collate of the case's graphs from its DeviceGraphStore (built once per module)"""
    if (family, case) not in _STORES:
        from esc_gnn_amd.datasets import build_feature_dataset
        raw = [E.Data(x=d["x"].clone(), edge_index=d["edge_index"].clone(), y=d["y"].clone(), num_nodes=d["num_nodes"],
                      edge_attr=d["edge_attr"].clone() if "edge_attr" in d else None) for d in ec.raw_graphs(family, case)]
        graphs = build_feature_dataset(raw, ec.HOPS, use_rd=True, self_loop=ec.SELF_LOOP[family])
        _STORES[(family, case)] = E.DeviceGraphStore(graphs, torch.device(DEV))
    store = _STORES[(family, case)]
    return store.collate(torch.arange(len(store)))


def product_model(E, family, L, H, state):
    if family == "count":
        m = E.NestedGIN_eff(None, L, H, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True)
    elif family == "zinc":
        from esc_gnn_amd.zinc_models import NestedGIN_eff
        m = NestedGIN_eff(None, L)
    else:
        from esc_gnn_amd.ogb_mol_gnn import GNN
        m = GNN("ogbg-molhiv", 1, num_layer=L, emb_dim=H, gnn_type="gin_eff", virtual_node=True, residual=True, drop_ratio=0.0,
                JK="last", graph_pooling="mean")
    assert list(m.state_dict().keys()) == list(state.keys())
    m.load_state_dict(state)
    return m.to(DEV).train()


def engine_of(E, family, model):
    from esc_gnn_amd.engine import OgbStepEngine, ZincStepEngine
    return {"count": E.StepEngine, "zinc": ZincStepEngine, "ogb": OgbStepEngine}[family](model)


def per_op(model):
    twin = copy.deepcopy(model)
    if hasattr(twin, "engine_forward"):
        twin.engine_forward = False
    else:
        twin.step_engine = False
    return twin.train()


def torch_loss(family, pred, b):
    if family == "ogb":
        return torch.nn.functional.binary_cross_entropy_with_logits(pred, b.y.float().view(-1, 1))
    return torch.nn.L1Loss()(pred, b.y.view(-1, 1))


def ops_loss(E, family, pred, b):
    if family == "ogb":
        return E.ops.bce_with_logits_loss(pred, b.y.float().view(-1, 1))
    return E.ops.l1_loss(pred, b.y)


def reduces_deferred(family, L):
    """Do the weight gradients of one step (csrc/engine_plan.h: 3L+6, 3L+3, 5L) fit the one reduce launch of 48 jobs?  Then
    esc_*_train_step takes the BatchNorm statistics of the main chain from the GEMM epilogues, as esc_*_forward_train always does,
    and the two forwards are the same launches.  Past it train_step takes them in passes of their own: another summation order,
    and the node's predictions are held to B like everything else instead of bit for bit to train_step's."""
    return {"count": 3 * L + 6, "zinc": 3 * L + 3, "ogb": 5 * L}[family] <= 48


def is_engine_node(pred):
    return pred.grad_fn is not None and type(pred.grad_fn).__name__.startswith("_EngineNode")


def grads_of(model):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in model.named_parameters()}


# ---- the bound -------------------------------------------------------------------------------------------------------------------
class Held(object):
    """holds values to B against one oracle step; prints every figure with its e_ref before it asserts anything"""

    def __init__(self, tag, step):
        self.tag, self.step, self.lines, self.bad = tag, step, [], []
        self.truth = dict(ec.float_items(step["fp64"]))
        self.e_ref = ec.reference_errors(step)
        self.worst = (0.0, None)

    def check(self, who, name, value):
        truth = self.truth[name]
        assert value is not None, (who, name)
        value = value.detach()
        assert bool(torch.isfinite(value).all()), (who, name)
        e, e_ref = ec.error(value, truth), self.e_ref[name]
        b = ec.bound(e_ref)
        d = value.double().cpu().reshape(truth.shape) - truth
        rel_f = float(d.norm()) / max(float(truth.double().norm()), 1e-12)
        self.lines.append("%-10s %-52s error %.3g  e_ref %.3g  bound %.3g%s"
                          % (who, name, e, e_ref, b, "" if e <= b else "  FAILS (relative Frobenius %.3g)" % rel_f))
        if e > b:
            self.bad.append((who, name, e, e_ref, rel_f))
        if e / b > self.worst[0]:
            self.worst = (e / b, "%s %s" % (who, name))

    def grads(self, who, grads, only=None):
        for n in self.step["fp64"]["grads"]:
            if only is None or only(n):
                self.check(who, "grad:" + n, grads[n])

    def buffers(self, who, model):
        mine = dict(model.named_buffers())
        for n, t in self.step["fp64"]["buffers"].items():
            if t.is_floating_point():
                self.check(who, "buf:" + n, mine[n])
            else:
                assert int(mine[n]) == int(t), (who, n, int(mine[n]), int(t))

    def done(self):
        print("\n".join(["--- %s" % self.tag] + self.lines))
        print("worst error / bound of %s: %.3g (%s)" % (self.tag, self.worst[0], self.worst[1]))
        assert not self.bad, self.bad


def finite(tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors if t is not None)


def bitwise(a, b, what):
    pa, la, ga = a
    pb, lb, gb = b
    assert torch.equal(pa, pb), (what, "predictions", int((pa != pb).sum()))
    assert torch.equal(la, lb), (what, "loss", float(la), float(lb))
    for n in ga:
        assert torch.equal(ga[n], gb[n]), (what, n, int((ga[n] != gb[n]).sum()))


def step_of(eng, model, b):
    loss, pred = eng.train_step(b, return_pred=True)
    out = (pred.detach().clone(), loss.detach().clone(), grads_of(model))
    torch.cuda.synchronize()
    return out


# ---- the batch itself ------------------------------------------------------------------------------------------------------
# (one node without self loops is a dataset without any edge: no batch to speak of)
_BATCHES = [(f, c) for c in ec.CASE_NAMES + ("single_node", "single_path3") for f in FAMILIES
            if ec.SELF_LOOP[f] or c != "single_node"]


@pytest.mark.parametrize("family,case", _BATCHES, ids=["%s-%s" % fc for fc in _BATCHES])
def test_product_batch_equals_oracle_batch(E, family, case):
    """Data list -> feature builder -> DeviceGraphStore -> collate: integer-equal to the batch the oracle steps on"""
    want = ec.oracle_batch(family, case)
    b = device_batch(E, family, case)
    assert b.num_graphs == want["num_graphs"]
    for k in ("edge_index", "pos_enc", "pos_index", "pos_batch", "batch"):
        assert torch.equal(b[k].cpu().to(want[k].dtype), want[k]), k
    assert torch.equal(b.x.cpu().reshape(want["x"].shape).to(want["x"].dtype), want["x"])
    assert torch.equal(b.y.cpu().reshape(-1), want["y"].reshape(-1))
    if "edge_attr" in want:
        assert torch.equal(b.edge_attr.cpu().reshape(want["edge_attr"].shape), want["edge_attr"])


# ---- every case, every family, both schedules ------------------------------------------------------------------------------
# ec.MODELS on every case, and the deep models of ec.DEEP (reduce jobs at and past what one launch takes: the last depth that
# defers its weight-gradient reduces, and the depths that reduce each at once out of its own slab region) on their one case each
# SCHEDULE_MODELS: values of the step schedule (csrc/engine_plan.h) that the models above do not reach.  count 2/64 is the one
# small depth where the node-activation fusion (H >= 64) and per-layer edge terms one layer ahead (L < 3) coincide; ogb 2/64 has
# both of its widths (H, 2H) on the GEMM-epilogue statistics.  The OGB model on `mixed` and `mixed_hub_last` only: its G = 2 cases
# are ill-conditioned (see ec.DEEP), and on `hub65` (G = 3, e_ref 2.3e-5 in convs.1.mlp.0.weight) the three-row BatchNorms of the
# virtual-node MLP put the PER-OP path at 1.19 B (grad mlp_virtualnode_list.0.0.weight 1.26e-5, e_ref 3.5e-6; the engine 1.05e-5
# against B = 1.06e-5), on both schedules and by the same figures with and without the schedule: `mixed_hub_last` took its place
# (worst e_ref 4.8e-6; 0.50 B on the device).
SCHEDULE_MODELS = (("count", 2, 64), ("ogb", 2, 64))
SCHEDULE_CASES = {"count": ("mixed", "minimal", "rows_65"), "ogb": ("mixed", "mixed_hub_last")}
_ON_CASE = ([(m, c) for c in ec.CASE_NAMES for m in ec.MODELS] + [(d[:3], d[3]) for d in ec.DEEP] +
            [(m, c) for m in SCHEDULE_MODELS for c in SCHEDULE_CASES[m[0]]])


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("model,case", _ON_CASE, ids=["%s-%s" % (ec.model_id(m), c) for m, c in _ON_CASE])
def test_engine_on_case(E, schedule_knobs, model, case, schedule):
    """train_step, its repeat, predict, the per-op twin and the engine as an autograd node on one case: see the module
    docstring for the bound.  `zero_variance`: every BatchNorm column has zero batch variance and the fp32 oracle cannot
    produce the gradients (test_engine_cases_cpu.py), so everything must be finite and the predictions within B."""
    family, L, H = model
    schedule_knobs.call("esc_engine_set_two_stream_min_edges", SCHEDULES[schedule])
    step = ec.oracle_step(family, case, L, H)
    with_grads = case != "zero_variance"
    held = Held("%s %s %s" % (ec.model_id(model), case, schedule), step)
    b = device_batch(E, family, case)
    mine = product_model(E, family, L, H, step["state"])
    twin, node = per_op(mine), copy.deepcopy(mine)

    # 1. the whole step as one call
    eng = engine_of(E, family, mine)
    first = step_of(eng, mine, b)
    assert finite([first[0], first[1]] + list(first[2].values()))
    held.check("train_step", "pred", first[0])
    if with_grads:
        held.check("train_step", "loss", first[1])
        held.grads("train_step", first[2])
        held.buffers("train_step", mine)
    else:
        assert finite(mine.buffers())
        assert all(int(c) == 1 for n, c in mine.named_buffers() if n.endswith("num_batches_tracked"))
    # 2. eval mode on the running statistics of that step
    ev = eng.predict(b)
    held.check("predict", "eval_pred", ev)
    # 3. the same step again, no optimiser step in between: scratch, partial sums and events are reused
    bitwise(first, step_of(eng, mine, b), "second train_step")
    # 4. the per-op path: a second implementation
    pt = twin(b)
    assert not is_engine_node(pt)
    lt = ops_loss(E, family, pt, b)
    lt.backward()
    held.check("per_op", "pred", pt)
    if with_grads:
        held.check("per_op", "loss", lt)
        held.grads("per_op", grads_of(twin))
    else:
        assert finite([lt] + list(grads_of(twin).values()))
    # 5. model(batch) in training mode: one autograd node on the engine, gradients through a torch loss
    pn = node(b)
    assert is_engine_node(pn)
    if reduces_deferred(family, L):
        assert torch.equal(pn.detach(), first[0])
    else:
        print("node predictions that differ from train_step's in some bit: %d of %d" % (int((pn.detach() != first[0]).sum()), pn.numel()))
        held.check("node", "pred", pn)
    ln = torch_loss(family, pn, b)
    ln.backward()
    if with_grads:
        held.check("node", "loss", ln)
        held.grads("node", grads_of(node))
        held.buffers("node", node)
    else:
        assert finite([ln] + list(grads_of(node).values()))
    held.done()


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("model", ec.MODELS, ids=ec.model_id)
def test_large_small_large_on_one_engine(E, schedule_knobs, model, schedule):
    """`mixed`, `minimal`, `mixed` again on ONE engine: the workspace, the bst_part / col_stats partials and the slab cursors
    of the large batch are still there when the small one runs.  The third result is bitwise the first, the second within B."""
    family, L, H = model
    schedule_knobs.call("esc_engine_set_two_stream_min_edges", SCHEDULES[schedule])
    big, small = ec.oracle_step(family, "mixed", L, H), ec.oracle_step(family, "minimal", L, H)
    mine = product_model(E, family, L, H, big["state"])
    eng = engine_of(E, family, mine)
    b_big, b_small = device_batch(E, family, "mixed"), device_batch(E, family, "minimal")
    first = step_of(eng, mine, b_big)
    second = step_of(eng, mine, b_small)
    third = step_of(eng, mine, b_big)
    bitwise(first, third, "large batch after the small one")
    held = Held("%s mixed->minimal->mixed %s" % (ec.model_id(model), schedule), small)
    held.check("after_big", "pred", second[0])
    held.check("after_big", "loss", second[1])
    held.grads("after_big", second[2])
    # predict of the small batch on the large batch's workspace too (the running statistics have seen three steps: finite only)
    assert finite([eng.predict(b_small)])
    held.done()
    held = Held("%s mixed (first of three) %s" % (ec.model_id(model), schedule), big)
    held.check("first", "pred", first[0])
    held.grads("first", first[2])
    held.done()


# ---- below the minimum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,H", [(3, 64), (1, 32)])
def test_counting_engine_refuses_one_node_and_stays_clean(E, L, H):
    """one one-node graph (N = 1, E = 1): refused on the host side of the library, nothing left open — the next step on
    `minimal` is bitwise the same step on a fresh engine built from the same state_dict"""
    step = ec.oracle_step("count", "minimal", L, H)
    b1 = device_batch(E, "count", "single_node")
    assert (b1.x.size(0), b1.edge_index.size(1), b1.num_graphs) == (1, 1, 1)
    mine = product_model(E, "count", L, H, step["state"])
    eng = E.StepEngine(mine)
    with pytest.raises(RuntimeError, match="needs >= 2 nodes and edges"):
        eng.train_step(b1)
    after = step_of(eng, mine, device_batch(E, "count", "minimal"))
    fresh_model = product_model(E, "count", L, H, step["state"])
    fresh = step_of(E.StepEngine(fresh_model), fresh_model, device_batch(E, "count", "minimal"))
    bitwise(after, fresh, "step after the refusal")
    assert all(torch.equal(a, c) for a, c in zip(mine.buffers(), fresh_model.buffers()))
    held = Held("count_L%d_H%d minimal after a refused batch" % (L, H), step)
    held.check("train_step", "pred", after[0])
    held.grads("train_step", after[2])
    held.done()


def test_zinc_single_graph_takes_the_per_op_path(E):
    """G = 1 (one path(3)): the engine is not ready (bn_lin1 over one row is skipped, which esc_zinc_* does not do), model(b)
    runs per op and is within B of the oracle, which skips bn_lin1 too"""
    from esc_gnn_amd.engine import zinc_engine_ready, zinc_engine_supports
    family, L, H = next(m for m in ec.MODELS if m[0] == "zinc")
    step = ec.oracle_step(family, "single_path3", L, H)
    b = device_batch(E, family, "single_path3")
    mine = product_model(E, family, L, H, step["state"])
    assert zinc_engine_supports(mine, b) and not zinc_engine_ready(mine, b)
    pred = mine(b)
    assert pred.grad_fn is not None and not is_engine_node(pred)
    loss = torch_loss(family, pred, b)
    loss.backward()
    held = Held("zinc single_path3 (G = 1)", step)
    held.check("per_op", "pred", pred)
    held.check("per_op", "loss", loss)
    got = grads_of(mine)
    held.grads("per_op", got)
    skipped = [n for n in got if n not in step["fp64"]["grads"]]
    assert skipped == ["bn_lin1.weight", "bn_lin1.bias"]
    assert all(got[n] is None or not bool(got[n].any()) for n in skipped)
    held.buffers("per_op", mine)
    mine.eval()
    with torch.no_grad():
        held.check("per_op", "eval_pred", mine(device_batch(E, family, "single_path3")))
    held.done()


def test_ogb_single_graph_takes_the_per_op_path(E):
    """G = 1 (one path(3)): ogb_engine_supports holds, but a batch of fewer than two graphs goes to the per-op path.  The
    reference cannot train on it (its virtual-node MLP normalises over the graphs and torch refuses one row), so the oracle
    comparison is the eval-mode forward; in training mode the per-op path must be the one taken, and it refuses the one row
    in the reference's own words."""
    from esc_gnn_amd.engine import ogb_engine_ready, ogb_engine_supports
    family, L, H = next(m for m in ec.MODELS if m[0] == "ogb")
    step = ec.oracle_step(family, "single_path3", L, H, train=False)
    b = device_batch(E, family, "single_path3")
    mine = product_model(E, family, L, H, step["state"])
    assert ogb_engine_supports(mine, b) and not ogb_engine_ready(mine, b)
    with pytest.raises(ValueError, match="more than 1 value per channel"):      # (the engine's refusal is a RuntimeError)
        mine(b)
    mine = product_model(E, family, L, H, step["state"]).eval()          # (the training forward moved running statistics)
    with torch.no_grad():
        ev = mine(b)
    held = Held("ogb single_path3 (G = 1)", step)
    held.check("per_op", "eval_pred", ev)
    held.done()


@pytest.mark.parametrize("family", ("zinc", "ogb"))
def test_two_graphs_are_enough_for_the_engine(E, family):
    """G = 2 (`minimal`) is the smallest batch of the graph-level heads: model(b) is the engine node and within B"""
    _, L, H = next(m for m in ec.MODELS if m[0] == family)
    step = ec.oracle_step(family, "minimal", L, H)
    b = device_batch(E, family, "minimal")
    assert b.num_graphs == 2
    mine = product_model(E, family, L, H, step["state"])
    pred = mine(b)
    assert is_engine_node(pred)
    loss = torch_loss(family, pred, b)
    loss.backward()
    held = Held("%s minimal (G = 2) as an autograd node" % family, step)
    held.check("node", "pred", pred)
    held.check("node", "loss", loss)
    held.grads("node", grads_of(mine))
    held.buffers("node", mine)
    held.done()
