"""The NGNN baseline without a GPU: tests/ngnn_oracle.py reproduces the three reference goldens written by
tools/make_golden_ngnn.py (integers and rd bit for bit, the model as test_qm9_cpu.py checks its own), and the run_zinc
command line takes `--model NGNN` while the baselines that stay out of scope still exit 1."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import ngnn_oracle as no


def subgraph_golden_cases():
    z = np.load(os.path.join(GOLDEN, "subgraphs_ngnn.npz"))
    for name in [str(s) for s in z["names"]]:
        n, h = (int(v) for v in z[name + "/meta"])
        yield name, n, z[name + "/in_edge_index"], h, {k: z[name + "/" + k] for k in
                                                         ("orig_node", "node_to_subgraph", "edge_index", "orig_edge", "z_spd", "z_drnl", "rd")}


def load_collate_ngnn3():
    z = np.load(os.path.join(GOLDEN, "collate_ngnn3.npz"))
    raws = [{k: z["raw%d_%s" % (j, k)] for k in ("x", "edge_index", "edge_attr", "y")} for j in range(int(z["num_graphs"]))]
    return raws, {k[len("batch_"):]: z[k] for k in z.files if k.startswith("batch_")}, int(z["h"])


def test_oracle_reproduces_subgraph_golden():
    names = []
    for name, n, ei, h, want in subgraph_golden_cases():
        got = no.expand_graph(n, ei[0], ei[1], h, use_rd=True)
        for k in ("orig_node", "node_to_subgraph", "edge_index", "orig_edge"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (name, k)
        assert np.array_equal(no.labels(got["z"], got["paths"], h, "spd"), want["z_spd"]), name
        assert np.array_equal(no.labels(got["z"], got["paths"], h, "drnl"), want["z_drnl"]), name
        assert np.array_equal(got["rd"].view(np.int32), want["rd"].view(np.int32)), name        # bit for bit: the same scipy call
        roots = got["sub_node_ptr"][:-1]
        assert np.array_equal(got["orig_node"][roots], np.arange(n)) and bool((got["rd"][roots] == 0).all()), name
        names.append(name)
    assert len(names) >= 10 and any("directed" in s for s in names) and "loops_repeats_h2" in names
    # the label list of a node reached over two frontier edges holds hop + 1 twice (utils.py:163-167): node 2 of a 4-cycle from root 0
    c4 = dict((c[0], c) for c in subgraph_golden_cases())["cycle4_h2"][4]
    first = c4["node_to_subgraph"] == 0
    assert c4["z_spd"][first].tolist() == [[1, 0], [2, 0], [2, 0], [3, 3]] and c4["z_drnl"][first].reshape(-1).tolist() == [1, 2, 2, 12]


def test_oracle_reproduces_collate_golden():
    raws, want, h = load_collate_ngnn3()
    got = no.expand_batch([r["x"].shape[0] for r in raws], [r["edge_index"] for r in raws], h, use_rd=True)
    for k in ("orig_node", "orig_edge", "node_to_subgraph", "edge_index", "batch"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(no.labels(got["z"], got["paths"], h, "spd"), want["z"])
    assert np.array_equal(np.concatenate([r["x"] for r in raws])[got["orig_node"]], want["x"])
    assert np.array_equal(np.concatenate([r["edge_attr"] for r in raws])[got["orig_edge"]], want["edge_attr"])
    assert np.array_equal(got["rd"].view(np.int32), want["rd"].reshape(-1).view(np.int32))
    assert want["rd"].shape == (want["x"].shape[0], 1) and want["z"].shape == (want["x"].shape[0], 2)
    n_all = sum(r["x"].shape[0] for r in raws)
    assert got["sub_node_ptr"].shape == (n_all + 1,) and int(got["sub_node_ptr"][-1]) == want["x"].shape[0]
    assert np.array_equal(want["subgraph_to_graph"], np.repeat(np.arange(len(raws)), [r["x"].shape[0] for r in raws]))


def ngnn_golden_runs():
    z = np.load(os.path.join(GOLDEN, "model_ngnn.npz"))
    _, b, _ = load_collate_ngnn3()
    b = {k: torch.tensor(v) for k, v in b.items()}
    for pooling in ("mean", "center"):
        for use_rd in (False, True):
            yield z, b, pooling, use_rd, "%s_%s" % (pooling, "rd" if use_rd else "nord")


def test_oracle_reproduces_model_golden():
    torch.set_num_threads(1)
    for z, b, pooling, use_rd, tag in ngnn_golden_runs():
        m = no.ngnn_from_recipe(z["seed"], z["layers"], pooling, use_rd).train()
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in z[tag + "/keys"]], tag
        assert ["x".join(map(str, v.shape)) or "scalar" for v in sd.values()] == [str(s) for s in z[tag + "/shapes"]], tag
        assert ("rd_projection_list.0.weight" in sd) == use_rd
        pred = m(*no.model_args(b))
        loss = torch.nn.functional.l1_loss(pred, torch.tensor(z["y"]))
        loss.backward()
        assert torch.equal(pred.detach(), torch.tensor(z[tag + "/pred"])) and float(loss.detach()) == float(z[tag + "/loss"]), tag
        for k, p in m.named_parameters():
            s, a = z[tag + "/gsum/" + k]
            g = p.grad.double()
            assert abs(float(g.sum()) - s) <= 1e-9 * max(1.0, a) and abs(float(g.abs().sum()) - a) <= 1e-9 * max(1.0, a), (tag, k)


def test_model_pooling_modes_differ_and_center_reads_the_root():
    z, b, _, _, _ = next(ngnn_golden_runs())
    assert not np.array_equal(z["mean_nord/pred"], z["center_nord/pred"])
    first = np.unique(b["node_to_subgraph"].numpy(), return_index=True)[1]
    assert np.array_equal(b["orig_node"].numpy()[first], np.arange(len(first)))        # the first node of a subgraph is its root


def test_cli_parser_accepts_ngnn():
    import esc_gnn_amd.run_zinc as rz
    a = rz.build_parser().parse_args("--model NGNN --h 2 --layers 2".split())
    assert a.model == "NGNN" and a.h == 2 and a.node_label == "spd" and a.use_rd is True
    assert hasattr(rz, "NGNN")


@pytest.mark.parametrize("model", ["I2GNN", "GNN"])
def test_cli_other_baselines_still_exit_1(model, capsys):
    import esc_gnn_amd.run_zinc as rz
    with pytest.raises(SystemExit) as e:
        rz.main(["--model", model])
    assert e.value.code == 1 and "Error: no such model!" in capsys.readouterr().out


def test_extension_header_is_bound_and_exported():
    """include/escgnn_subgraphs.h, as tests/test_abi.py holds escgnn_hip.h: read by the same strict reader, every declared
    symbol exported by the library and bound by lib(); and it shares no name with the main header's pinned binding"""
    import ctypes
    import re
    from esc_gnn_amd import _abi, _native as nv
    text = re.sub(r"/\*.*?\*/", "", open(nv.EXTENSION_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(esc_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["esc_segment_first_bwd", "esc_segment_first_fwd", "esc_subgraph_count", "esc_subgraph_fill"]
    ext = _abi.load(nv.EXTENSION_HEADER)
    assert sorted(ext.functions) == declared == sorted(nv.EXTENSION_SIGNATURES) and not ext.structs and not ext.constants
    assert not set(declared) & set(nv.SIGNATURES)
    h, raw = nv.lib(), ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
        assert list(getattr(h, name).argtypes) == list(nv.EXTENSION_SIGNATURES[name]) and getattr(h, name).restype is ctypes.c_int
