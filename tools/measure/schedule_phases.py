"""Phase marks of the flagship step under several esc_engine_set_side_stream modes, in ONE process (same dataset, same seed):
    ESC_PHASE_TIMING=1 python tools/measure/schedule_phases.py TAG MODE[,MODE...]
MODE -1 leaves the library default.  150 steps per mode; the marks are averaged over the last 127.  The last column says whether
the parameters after those steps equal the first mode's bit for bit.  ESC_ROOT=<other checkout> measures that tree's build instead
(A/B against a parent commit).  -> profiles/step_schedule_measurements.txt"""
import sys, os, ctypes, torch
root = os.environ.get("ESC_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [root]
import esc_gnn_amd as E
from esc_gnn_amd import _native as nv
from esc_gnn_amd.datasets import build_count_dataset
tag = sys.argv[1]
modes = [int(v) for v in sys.argv[2].split(",")]
DEV = "cuda:0"
bs = 128
graphs = build_count_dataset(0, 4 * bs, h=3, use_rd=True, self_loop=True)
y = torch.cat([g.y.view(-1) for g in graphs])
for g in graphs:
    g.y = (g.y.view(-1) - y.mean()) / y.std()
store = E.DeviceGraphStore(graphs, DEV)
ids = [torch.arange(i * bs, (i + 1) * bs) for i in range(4)]
ref = None
for mode in modes:
    if mode >= 0:
        nv.call("esc_engine_set_side_stream", mode)
    torch.manual_seed(0)
    m = E.NestedGIN_eff(None, 4, 256, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True).to(DEV)
    opt = E.optim.FlatAdam(m.parameters(), lr=1e-3, late=E.parallel.edge_pipeline_parameters(m))     # bench.py's optimiser
    m.train()
    eng = E.StepEngine(m)
    nxt = store.collate(ids[0])
    for i in range(150):
        b = nxt
        eng.begin_step(b)
        nxt = store.collate(ids[(i + 1) % 4])
        eng.end_step()
        opt.step()
    torch.cuda.synchronize()
    out = (ctypes.c_double * 6)()
    n = nv.lib().esc_engine_phase_times(out, 0)
    par = opt.flat_param.clone()
    if ref is None:
        ref = par
    print("%s mode %4d: n=%d edge_fwd %.1f | node_fwd %.1f | node_bwd %.1f | nodebwd->edgebwd %.1f | start->end %.1f | end->start %.1f | same_as_first %s"
          % ((tag, mode, n) + tuple(v * 1e3 for v in out) + (bool(torch.equal(par, ref)),)), flush=True)
