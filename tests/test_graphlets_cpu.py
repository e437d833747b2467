"""The graphlet-label oracle (tests/graphlet_oracle.py) against hand-counted graphs and the closed forms on complete
graphs, and the CLI surface the labels add to run_graphcount.  No GPU."""
import numpy as np
import pytest

import graphlet_oracle as go


def test_oracle_hand_cases():
    for name, n, ei, want in go.hand_cases():
        assert np.array_equal(go.orbit_labels(n, ei), want), name


def test_oracle_pattern_graphs_hold_one_copy_of_themselves():
    n, ei = go.pattern_edges("tailed_triangle")          # the paw: node 0 carries the tail, node 3 ends it
    got = go.orbit_labels(n, ei)
    assert got[:, :3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1]]
    assert not got[:, 3:6].any() and not got[:, 8:].any()
    n, ei = go.pattern_edges("chordal_cycle")            # the diamond: chord 0-2
    got = go.orbit_labels(n, ei)
    assert got[:, 3:5].tolist() == [[1, 0], [0, 1], [1, 0], [0, 1]]
    assert not got[:, 5].any() and not got[:, 8:].any()
    assert go.orbit_sums(got)[:, 1].tolist() == [1, 1, 1, 1]
    n, ei = go.pattern_edges("4_path")
    got = go.orbit_labels(n, ei)
    assert got[:, 6].tolist() == [1, 0, 0, 1] and got[:, 7].tolist() == [0, 1, 1, 0]
    assert not np.delete(got, [6, 7], axis=1).any()


def test_oracle_normalises_messy_input():
    n, messy, clean = go.messy_case()
    got = go.orbit_labels(n, messy)
    assert np.array_equal(got, go.orbit_labels(n, clean))
    assert got.any() and not got[5].any()                # node 5 is isolated


@pytest.mark.parametrize("n", [4, 5, 6, 13])
def test_oracle_complete_graph_closed_forms(n):
    got = go.orbit_labels(n, go.complete_graph_edges(n))
    assert np.array_equal(got, np.tile(go.complete_graph_row(n), (n, 1)))


def test_complete_graph_row_hand_values():
    assert go.complete_graph_row(4).tolist() == [3, 6, 3, 3, 3, 1, 6, 6, 0, 0, 0]
    assert go.complete_graph_row(5).tolist() == [12, 24, 12, 12, 12, 4, 24, 24, 12, 24, 24]
    assert int(go.complete_graph_row(64)[8:].sum()) == 60 * 7624512 * 5 // 64 == 35739900 < 2 ** 31   # houses in K64


def test_new_flags_and_unchanged_defaults():
    import esc_gnn_amd.run_graphcount as rg
    a = rg.build_parser().parse_args([])
    assert a.synthetic_labels == "triangle" and a.graphlet_orbit == -1
    want = dict(model="NestedGIN_eff", target=3, ab=False, layers=5, h=3, max_nodes_per_hop=None, node_label="hop",
                epochs=2000, batch_size=256, lr=1e-3, lr_decay_factor=0.9, patience=10, normalize_x=False,
                not_normalize_dist=False, RNI=False, use_relative_pos=False, seed=0, save_appendix="",
                keep_old=False, dataset="count_cycle", load_model=None, eval=0, train_only=0, synthetic_graphs=5000,
                data_root="data")
    for k, v in want.items():
        assert getattr(a, k) == v, k
    b = rg.build_parser().parse_args("--dataset count_graphlet --target 4 --synthetic_labels task --graphlet_orbit 2".split())
    assert (b.dataset, b.target, b.synthetic_labels, b.graphlet_orbit) == ("count_graphlet", 4, "task", 2)
    with pytest.raises(SystemExit):
        rg.build_parser().parse_args("--synthetic_labels other".split())


def test_task_label_column_selection_and_ranges():
    from esc_gnn_amd.graphlets import GRAPHLET_NAMES, GRAPHLET_ORBITS
    from esc_gnn_amd.run_graphcount import task_label_column
    assert GRAPHLET_ORBITS == go.ORBITS and GRAPHLET_NAMES == tuple(p[0] for p in go.PATTERNS)
    assert [task_label_column("count_cycle", t) for t in range(4)] == [("cycles", t) for t in range(4)]
    assert [task_label_column("count_graphlet", t) for t in range(5)] == [("graphlets", t) for t in range(5)]
    for t, cols in enumerate(GRAPHLET_ORBITS):
        assert [task_label_column("count_graphlet", t, k) for k in range(len(cols))] == [("graphlet_orbits", c) for c in cols]
    for bad in (("count_graphlet", 5, -1), ("count_graphlet", -1, -1), ("count_cycle", 4, -1), ("count_graphlet", 1, 2),
                ("count_graphlet", 2, 1), ("count_graphlet", 0, -2), ("count_cycle", 0, 1), ("count_other", 0, -1)):
        with pytest.raises(ValueError):
            task_label_column(*bad)
    with pytest.raises(ValueError, match=r"0\.\.4"):
        task_label_column("count_graphlet", 5)
    with pytest.raises(ValueError, match=r"0\.\.3"):
        task_label_column("count_cycle", 4)
    with pytest.raises(ValueError, match=r"0\.\.1"):
        task_label_column("count_graphlet", 1, 2)


# ---- the packing and the status decoder the label wrappers share (esc_gnn_amd/ragged.py) --------------------------------
def test_shared_edge_list_packing():
    import torch
    from esc_gnn_amd.ragged import pack_edge_lists, split_rows
    none = torch.zeros((2, 0), dtype=torch.int64)
    tri = torch.tensor([[0, 1, 2], [1, 2, 0]])
    node_ptr, edge_ptr, ends = pack_edge_lists([4, 0, 3], [none, none, tri])
    assert node_ptr.tolist() == [0, 4, 4, 7] and edge_ptr.tolist() == [0, 0, 0, 3]
    assert ends.dtype == node_ptr.dtype == edge_ptr.dtype == torch.int64 and torch.equal(ends, tri)
    flat = pack_edge_lists([4, 0, 3], [none, none.reshape(-1), tri.reshape(-1).to(torch.int32)])      # 2m entries: taken as [2, m]
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(flat, (node_ptr, edge_ptr, ends)))
    rows = torch.arange(7 * 4).view(7, 4)
    parts = split_rows(rows, node_ptr)
    assert [p.shape for p in parts] == [(4, 4), (0, 4), (3, 4)] and torch.equal(torch.cat(parts), rows)
    node_ptr, edge_ptr, ends = pack_edge_lists([], [])                               # the empty call
    assert node_ptr.tolist() == [0] and edge_ptr.tolist() == [0] and ends.shape == (2, 0)
    assert split_rows(torch.zeros(0, 4), node_ptr) == []


def test_shared_status_decoder_names_the_first_offending_graph():
    import torch
    from esc_gnn_amd.ragged import ESC_ERANGE, MAX_NODES, raise_for_status
    assert MAX_NODES == 64 and ESC_ERANGE != 0
    node_ptr = torch.tensor([0, 3, 68, 70, 75])
    raise_for_status("cycle_counts", "cycle", torch.zeros(4, dtype=torch.int32), node_ptr)             # all ESC_OK: nothing
    raise_for_status("cycle_counts", "cycle", torch.zeros(0, dtype=torch.int32), torch.tensor([0]))
    other = 1 if ESC_ERANGE != 1 else 2
    with pytest.raises(ValueError, match=r"^cycle_counts: graph 1 has 65 nodes; the cycle-count kernel takes graphs of at most 64 nodes$"):
        raise_for_status("cycle_counts", "cycle", torch.tensor([0, ESC_ERANGE, other, ESC_ERANGE], dtype=torch.int32), node_ptr)
    with pytest.raises(ValueError, match=r"^graphlet_counts: graph 2 has a node id outside \[0, 2\)$"):
        raise_for_status("graphlet_counts", "graphlet", torch.tensor([0, 0, other, ESC_ERANGE], dtype=torch.int32), node_ptr)
    with pytest.raises(ValueError, match=r"^graphlet_counts: graph 3 has a node id outside \[0, 5\)$"):     # any other non-zero code
        raise_for_status("graphlet_counts", "graphlet", torch.tensor([0, 0, 0, -7], dtype=torch.int32), node_ptr)
