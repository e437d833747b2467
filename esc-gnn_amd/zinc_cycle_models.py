"""ZINC cycle counting: NestedGIN_eff of the reference's zinc_cycle_models.py:506-613, the node-level twin of
zinc_models.NestedGIN_eff.  The two class bodies differ in one line: the cycle model drops global_add_pool, so lin1 reads
cat(xs) row by row, bn_lin1 normalises over the nodes and lin2 predicts one value per node (the 3..6-cycles through it,
run_zinc_cycle.py).  Same constructor, parameters and state_dict keys as zinc_models.NestedGIN_eff; the training and eval
forwards run through the ZINC step engine with node_readout = 1 (csrc/engine.hip esc_zinc_*)."""
import torch.nn.functional as F

from . import zinc_models


class NestedGIN_eff(zinc_models.NestedGIN_eff):
    node_readout = True            # esc_zinc_gin_t.node_readout: pred / y / loss per node

    def _readout(self, states, data):
        o = self.lin1(states)                              # reference :601-602: no pooling
        o = self.bn_lin1(o) if o.size(0) > 1 else F.elu(o)  # :603-607 (dropout p = 0; ELU fused into the BatchNorm)
        return self.lin2(o)
