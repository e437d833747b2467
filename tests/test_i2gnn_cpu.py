"""The I2GNN baseline without a GPU: tests/i2gnn_oracle.py reproduces the three reference goldens written by
tools/make_golden_i2gnn.py (integers and rd bit for bit, the fp32 model bit for bit), a 4-cycle written out by hand, the
state_dict layout of zinc_cycle_models.I2GNN, the binding of include/escgnn_i2gnn.h, and the run_zinc_cycle command line."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import i2gnn_oracle as io

INT_FIELDS = ("orig_node", "z", "node_to_subgraph2", "subgraph2_to_subgraph", "center_idx", "edge_index", "orig_edge")


def subgraph2_golden_cases():
    z = np.load(os.path.join(GOLDEN, "subgraphs_i2gnn.npz"))
    for name in [str(s) for s in z["names"]]:
        n, h = (int(v) for v in z[name + "/meta"])
        yield name, n, z[name + "/in_edge_index"], h, {k: z[name + "/" + k] for k in INT_FIELDS + ("rd",)}


def load_collate_i2gnn3():
    z = np.load(os.path.join(GOLDEN, "collate_i2gnn3.npz"))
    raws = [{k: z["raw%d_%s" % (j, k)] for k in ("x", "edge_index", "edge_attr", "y")} for j in range(int(z["num_graphs"]))]
    return raws, {k[len("batch_"):]: z[k] for k in z.files if k.startswith("batch_")}, int(z["h"])


def i2gnn_golden_runs():
    z = np.load(os.path.join(GOLDEN, "model_i2gnn.npz"))
    _, b, _ = load_collate_i2gnn3()
    b = {k: torch.tensor(v) for k, v in b.items()}
    for tag in io.CONFIGS:
        yield z, b, tag


def test_oracle_reproduces_subgraph2_golden():
    names = []
    for name, n, ei, h, want in subgraph2_golden_cases():
        got = io.expand_graph2(n, ei[0], ei[1], h, use_rd=True)
        for k in INT_FIELDS:
            assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k)
        assert want["rd"].shape == (want["z"].shape[0], 2) and want["z"].shape[1] == 4
        assert np.array_equal(got["rd"].view(np.int32), want["rd"].view(np.int32)), name        # bit for bit: the same scipy call
        # the first row of every copy is its root, at resistance 0 of itself; the side row is at resistance 0 in column 1
        ci = got["center_idx"]
        assert np.array_equal(ci[:, 0], got["s2_node_ptr"][:-1]) and np.array_equal(got["orig_node"][ci[:, 0]], got["subgraph2_to_subgraph"])
        assert bool((got["rd"][ci[:, 0], 0] == 0).all()) and bool((got["rd"][ci[:, 1], 1] == 0).all()), name
        assert bool((np.diff(got["node_to_subgraph2"]) >= 0).all()) and bool((np.diff(got["subgraph2_to_subgraph"]) >= 0).all())
        assert int(got["z"].max()) <= 2 * h + 5
        names.append(name)
    assert len(names) >= 12 and "selfloops_only_h2" in names and "directed_ring_h5" in names and "isolated_h2" in names
    cases = dict((c[0], c) for c in subgraph2_golden_cases())
    # a root with no neighbour: one copy, its label pair tiled twice without the shift, centre == side
    iso = cases["isolated_h2"][4]
    assert iso["z"][0].tolist() == [1, 0, 1, 0] and iso["center_idx"][0].tolist() == [0, 0] and iso["rd"][0].tolist() == [0, 0]
    # a root whose only edges are two self loops: two copies of one node, neighbour = the root itself
    sl = cases["selfloops_only_h2"][4]
    assert sl["z"][:2].tolist() == [[1, 0, 1 + 5, 0 + 5]] * 2 and sl["center_idx"][:2].tolist() == [[0, 0], [1, 1]]
    assert sl["subgraph2_to_subgraph"][:2].tolist() == [0, 0]
    # the directed ring: the second root is further from some node than the first (the walk goes the long way round)
    dr = cases["directed_ring_h5"][4]
    assert bool((dr["z"][:, 2] - 8 > dr["z"][:, 0]).any())


def test_four_cycle_by_hand():
    """0-1-2-3-0 at h = 2: every root sees all four nodes and has two neighbours, so 4 roots x 2 copies x 4 nodes."""
    ei = np.array([[0, 1, 2, 3, 1, 2, 3, 0], [1, 2, 3, 0, 0, 1, 2, 3]], dtype=np.int64)
    got = io.expand_graph2(4, ei[0], ei[1], 2, use_rd=True)
    assert got["z"].shape == (32, 4) and got["center_idx"].shape == (8, 2) and got["edge_index"].shape == (2, 64)
    assert got["subgraph2_to_subgraph"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert got["sub_node_ptr"].tolist() == [0, 8, 16, 24, 32] and got["sub2_ptr"].tolist() == [0, 2, 4, 6, 8]
    # root 0: canonical order 0 | 1, 3 | 2; its sub-edges that leave it are 0->1 (edge 0) and 0->3 (edge 7): neighbours 1, then 3
    assert got["orig_node"][:8].tolist() == [0, 1, 3, 2, 0, 1, 3, 2]
    assert got["center_idx"][:2].tolist() == [[0, 1], [4, 6]]
    root_pair = [[1, 0], [2, 0], [2, 0], [3, 3]]                       # node 2 is entered over two frontier edges
    assert got["z"][:4, :2].tolist() == root_pair and got["z"][4:8, :2].tolist() == root_pair
    # copy 0, neighbour 1: distances from 1 are 0:1, 1:0, 3:2 (two paths), 2:1 -> pairs + h + 3 = + 5
    assert got["z"][:4, 2:].tolist() == [[2 + 5, 0 + 5], [1 + 5, 0 + 5], [3 + 5, 3 + 5], [2 + 5, 0 + 5]]
    for s2 in range(8):                                               # the neighbour root of every copy is labelled [1, 0] + 5
        assert got["z"][got["center_idx"][s2, 1], 2:].tolist() == [1 + 5, 0 + 5]
    # resistance distances of the 4-cycle: 3/4 between neighbours, 1 across
    assert np.allclose(got["rd"][:4], [[0, 0.75], [0.75, 0], [0.75, 1.0], [1.0, 0.75]], atol=1e-6)


def test_oracle_reproduces_collate_golden():
    raws, want, h = load_collate_i2gnn3()
    got = io.expand_batch2([r["x"].shape[0] for r in raws], [r["edge_index"] for r in raws], h, use_rd=True)
    for k in ("orig_node", "orig_edge", "z", "node_to_subgraph2", "subgraph2_to_subgraph", "center_idx", "edge_index", "batch",
              "subgraph_to_graph"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["orig_node"], want["node_to_original_node"])
    assert np.array_equal(np.concatenate([r["x"] for r in raws])[got["orig_node"]], want["x"])
    assert np.array_equal(np.concatenate([r["edge_attr"] for r in raws])[got["orig_edge"]], want["edge_attr"])
    assert np.array_equal(got["rd"].view(np.int32), want["rd"].view(np.int32))
    assert np.array_equal(np.concatenate([r["y"] for r in raws]), want["y"]) and want["y"].shape[1] == 4
    assert want["x"].shape[0] == 2023 and want["edge_index"].shape[1] == 4052 and want["center_idx"].shape[0] == 154
    assert not bool((np.diff(want["node_to_original_node"]) >= 0).all())          # NOT sorted: the context mean needs a grouping


def test_oracle_reproduces_model_golden():
    torch.set_num_threads(1)
    for z, b, tag in i2gnn_golden_runs():
        m = io.i2gnn_from_recipe(z["seed"], z["layers"], tag).train()
        pred = m(b)
        loss = torch.nn.functional.l1_loss(pred, torch.tensor(z["y"]))
        loss.backward()
        assert pred.shape == (int(b["subgraph_to_graph"].numel()), 1)                  # node level
        assert torch.equal(pred.detach(), torch.tensor(z[tag + "/pred"])) and float(loss.detach()) == float(z[tag + "/loss"]), tag
        for k, p in m.named_parameters():
            if p.grad is None:             # built and never read: rd_projection; without a gate, the last z table / rd projection
                assert k.split(".")[0] in ("rd_projection", "z_embedding_list", "rd_projection_list"), (tag, k)
                assert tag + "/gsum/" + k not in z.files, (tag, k)
                continue
            s, a = z[tag + "/gsum/" + k]
            g = p.grad.double()
            assert abs(float(g.sum()) - s) <= 1e-9 * max(1.0, a) and abs(float(g.abs().sum()) - a) <= 1e-9 * max(1.0, a), (tag, k)


@pytest.mark.parametrize("tag", list(io.CONFIGS))
def test_i2gnn_state_dict_layout(tag):
    """keys and shapes of the device model against the recorded ones of the reference class; nothing touches a device"""
    from esc_gnn_amd.zinc_cycle_models import I2GNN
    z = np.load(os.path.join(GOLDEN, "model_i2gnn.npz"))
    m = I2GNN(None, num_layers=int(z["layers"]), **io.CONFIGS[tag])
    sd = m.state_dict()
    assert all(v.device.type == "cpu" for v in sd.values())
    assert list(sd.keys()) == [str(k) for k in z[tag + "/keys"]]
    assert ["x".join(map(str, v.shape)) or "scalar" for v in sd.values()] == [str(s) for s in z[tag + "/shapes"]]
    assert ("subgraph_gate.0.0.weight" in sd) == io.CONFIGS[tag]["gate"]
    assert ("double_nns.0.0.weight" in sd) == io.CONFIGS[tag]["double_pooling"]
    m.load_state_dict(io.i2gnn_from_recipe(z["seed"], z["layers"], tag).state_dict())


def test_i2gnn_every_pooling_combination_constructs():
    from esc_gnn_amd.zinc_cycle_models import I2GNN
    for p1 in ("mean", "add", "mean-context"):
        for p2 in ("mean", "add", "center", "mean-center", "mean-center-side"):
            s2 = {"mean-center": 2, "mean-center-side": 3}.get(p2, 1) + (p1 == "mean-context")
            m = I2GNN(None, num_layers=1, subgraph_pooling=p1, subgraph2_pooling=p2, double_pooling=True)
            assert m.fc1.in_features == 64 * s2 and m.double_nns[0][0].in_features == 64 * (1 + s2)
    with pytest.raises(ValueError):
        I2GNN(None, subgraph2_pooling="max")
    for kw in (dict(use_pos=True), dict(RNI=True), dict(use_virtual_node=True)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            I2GNN(None, **kw)


def test_i2gnn_header_is_bound_and_exported():
    """include/escgnn_i2gnn.h: read by the same strict reader as the other two headers, every declared symbol exported by the
    library and bound by lib(), no name shared with them; the NGNN header keeps its four names"""
    import ctypes
    import re
    from esc_gnn_amd import _abi, _native as nv
    text = re.sub(r"/\*.*?\*/", "", open(nv.I2GNN_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(esc_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["esc_pool_mean_center_side_bwd", "esc_pool_mean_center_side_fwd", "esc_sigmoid_mul_bwd",
                        "esc_sigmoid_mul_fwd", "esc_subgraph2_count", "esc_subgraph2_fill"]
    ext = _abi.load(nv.I2GNN_HEADER)
    assert sorted(ext.functions) == declared == sorted(nv.I2GNN_SIGNATURES) and not ext.structs and not ext.constants
    assert not set(declared) & set(nv.SIGNATURES) and not set(declared) & set(nv.EXTENSION_SIGNATURES)
    assert sorted(nv.EXTENSION_SIGNATURES) == ["esc_segment_first_bwd", "esc_segment_first_fwd", "esc_subgraph_count",
                                               "esc_subgraph_fill"]
    h, raw = nv.lib(), ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
        assert list(getattr(h, name).argtypes) == list(nv.I2GNN_SIGNATURES[name]) and getattr(h, name).restype is ctypes.c_int


def test_cli_parser_accepts_i2gnn():
    import esc_gnn_amd.run_zinc_cycle as rc
    a = rc.build_parser().parse_args("--model I2GNN --h 2 --layers 2".split())
    assert a.model == "I2GNN" and a.subgraph_pooling == "mean-context" and a.subgraph2_pooling == "mean-center-side"
    assert a.gate is True and a.double_pooling is True and a.use_rd is True and hasattr(rc, "I2GNN")


@pytest.mark.parametrize("model", ["GNN", "NGNN"])
def test_cli_other_baselines_still_exit_1(model, capsys):
    import esc_gnn_amd.run_zinc_cycle as rc
    with pytest.raises(SystemExit) as e:
        rc.main(["--model", model])
    assert e.value.code == 1 and "Error: no such model!" in capsys.readouterr().out


@pytest.mark.parametrize("flags,name", [(["--self_loop"], "self_loop"), (["--max_nodes_per_hop", "5"], "max_nodes_per_hop"),
                                        (["--node_label", "drnl"], "node_label"), (["--h", "48"], "h=48")])
def test_cli_i2gnn_refuses_what_has_no_path(flags, name):
    import esc_gnn_amd.run_zinc_cycle as rc
    with pytest.raises((NotImplementedError, ValueError), match=name):
        rc.main(["--model", "I2GNN"] + flags)
