"""What the NestedGIN twins share: the size of the ESC label table, the Sequential blocks the reference classes spell out
inline, the raw edge term, the conv1 / convs stack and the order-preserving reset.  nn.py is the layer library; the model
files (run_graphcount, kernel_gin, zinc_models, zinc_cycle_models, qm9_models, csl_models, expressive_models, ogb_mol_gnn)
keep their class names, constructors and what is theirs alone: inputs, edge attributes, readout and head.

Every block builds the module tree of the reference class child for child (the Absorbed* placeholders keep the indices of
the activations that the BatchNorm kernels fuse), and draws its parameters in the reference's order.
"""
from torch.nn import Dropout, ModuleList, Sequential

from . import ops
from .nn import AbsorbedELU, AbsorbedReLU, BatchNorm1d, GINEConv, Linear

Z_TABLE_ROWS = 1800  # reference run_graphcount.py:51 — always 1800, even for the 1700-wide no-rd layout

_ABSORBED = {"relu": AbsorbedReLU, "elu": AbsorbedELU}


def bn_act(hidden, act="relu"):
    """BatchNorm1d fused with the activation that follows it, and that activation's placeholder"""
    return BatchNorm1d(hidden, fuse_relu=act), _ABSORBED[act]()


def mlp(n_in, hidden, p, act="relu"):
    """Linear, Dropout, BN, act, Linear, Dropout, BN, act: children 0..7 (reference run_graphcount.py:77-89)"""
    return Sequential(Linear(n_in, hidden), Dropout(p), *bn_act(hidden, act),
                      Linear(hidden, hidden), Dropout(p), *bn_act(hidden, act))


def plain_conv(n_in, hidden, act):
    """GINEConv over Linear, act, Linear, act with no BatchNorm and a constant eps (reference run_sr.py:146-163,
    run_csl.py:152-169); `act`: the activation's module class"""
    return GINEConv(Sequential(Linear(n_in, hidden), act(), Linear(hidden, hidden), act()), train_eps=False, edge_dim=hidden)


def z_embedding(hidden, act="relu", dropout=None):
    """[Dropout,] BN, act, Linear, [Dropout,] BN, act; dropout=None: the five-child shape of the expressiveness and CSL
    models, which has no Dropout entries"""
    drop = (lambda: ()) if dropout is None else (lambda: (Dropout(dropout),))
    return Sequential(*drop(), *bn_act(hidden, act), Linear(hidden, hidden), *drop(), *bn_act(hidden, act))


def edge_term(z_initial, data, plan):
    """raw edge term z before any z_embedding: the dense `edge_pos` layout of the slow variant (reference
    run_graphcount.py:142-145) as a GEMM with the table, or the ESC bag over the table's rows"""
    if "edge_pos" in data:
        return ops.linear(data.edge_pos.float(), z_initial.weight.t().contiguous())
    return ops.esc_bag(z_initial.weight, plan)


def conv_stack(model, x, edge_index, z, plan, skip=None):
    """per-layer states [conv1(x), convs[0](.), ...].  `skip`: a module applied to x whose output leads the list — the
    counting model's x_embedding, the one caller.  It is a parameter here and not a line there because the reference
    launches it between conv1 and convs[0] (run_graphcount.py:161-169), and the launch order is kept."""
    h = model.conv1(x, edge_index, z, plan)
    xs = [h] if skip is None else [skip(x), h]
    for conv in model.convs:
        h = conv(h, edge_index, z, plan)
        xs.append(h)
    return xs


def reset_parameters(model, *names):
    """reset the named children in the order given — the order decides which random numbers each parameter draws.  A
    Sequential or ModuleList is reset child by child; children without reset_parameters are passed over."""
    for name in names:
        part = getattr(model, name)
        for layer in (part if isinstance(part, (Sequential, ModuleList)) else (part,)):
            if hasattr(layer, "reset_parameters"):
                layer.reset_parameters()
