"""Drop-in for the reference's models/stgcn_debug.py: `Model(num_classes=60)` called as `model(x, training)` -- ST-GCN whose blocks
contract with a trainable adjacency PER FRAME (SGTACN, models/stgcn_debug.py:118-145: einsum 'nkctv,ktvw->nctw'), one table
`l{i}.adjacency_matrix` of shape (3, T_i, 25, 25) per block, initialised to Graph().A repeated over the block's input frames
(`main_gnn.py --model stgcn_debug --freeze-graph-until E`: the tables are trained only while epoch > E).

x: (N, in_channels=3, T=frames, V=25, M) float32 on the GPU -> logits (N, num_classes).
The arithmetic runs in libsar_hip.so through sar_amd.stgcn_ta.STGCNTA; this module adapts it to torch.nn.Module / autograd exactly
like models/stpgcn.py does.  `trainable_adjacency` is accepted for main_gnn.py's sake: this model always owns its tables.
"""
import torch

from sar_amd.stgcn_ta import STGCNTA  # noqa: F401
from models.stgcn import _STGCNFunction, _Variable


class Model(torch.nn.Module):
    def __init__(self, num_classes=60, in_channels=3, device="cuda", seed=0, stream="joint", mfma="fp32",
                 trainable_adjacency=True, frames=300):
        super().__init__()
        assert stream in ("joint", "bone", "joint_motion", "bone_motion"), stream
        assert mfma == "fp32", "models.stgcn_debug runs in fp32"
        from sar_amd.bone import NTU_BONE_PAIRS
        self.engine = STGCNTA(num_classes=num_classes, in_channels=in_channels, device=device, seed=seed, frames=frames,
                              bone_pairs=NTU_BONE_PAIRS if stream.startswith("bone") else None, motion=stream.endswith("motion"))
        self._names = list(self.engine.shapes)
        for k in self._names:
            self.register_parameter(k.replace(".", "_"), torch.nn.Parameter(self.engine.p[k]))

    @property
    def trainable_variables(self):
        return [_Variable(k, getattr(self, k.replace(".", "_"))) for k in self._names]

    @property
    def variables(self):
        return self.trainable_variables

    @property
    def adjacency_matrices(self):
        """the per-block tables, (3, T_i, 25, 25) each"""
        return [getattr(self, self.engine.table_name(i).replace(".", "_")) for i in range(len(self.engine.blocks))]

    def forward(self, x, training=None):
        if training is None:
            training = self.training
        params = [getattr(self, k.replace(".", "_")) for k in self._names]
        if training and torch.is_grad_enabled():
            return _STGCNFunction.apply(x, self.engine, True, *params)
        return self.engine.forward(x, training=training)

    def train_step(self, x, labels, lr, global_batch_size=None, momentum=0.9):
        logits, loss = self.engine.loss_and_grad(x, labels, global_batch_size)
        self.engine.sgd_step(lr, momentum)
        return logits, loss
