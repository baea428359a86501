"""ST-GCN with a trainable adjacency per FRAME and per block: the reference's models/stgcn_debug.py on the HIP kernels.  The network
is ST-GCN's (same 10 blocks, data_bn prologue, head and residual kinds: sar_amd/stgcn.py); every block's spatial operator is SGTACN
(models/stgcn_debug.py:118-145):

    y3 = Conv2D(3F, 1x1)(x);   out = einsum('nkctv,ktvw->nctw', y3, A_i)         A_i: (K, T_i, V, V), trainable, owned by block i

with A_i initialised to Graph().A repeated over the block's T_i input frames (300 x 5, 150 x 3, 75 x 2 for a 300-frame clip).  The
variables are named `l{i}.adjacency_matrix`: main_gnn.py's --freeze-graph-until filters on that name, `train_adjacency` is its
per-step switch.  Block forward / backward are the dense path of STGCN (conv_gemm with taps = 1, the contraction,
_graph_backward_dense) with the three contractions on csrc/graph_dense_t.hip.  Block i's table follows l{i}.* in the flat buffer and
its gradient is written by block i's backward, so it is complete when the gradient bucket that holds it is handed to the all-reduce.
fp32 only.
"""
import numpy as np
import torch

from . import ops
from .stgcn import STGCN, BLOCKS, KS, KT, same_pad


def block_frames(frames, blocks):
    """input frame count of every block (TF 'SAME' temporal convolutions, stride s)"""
    out, T = [], int(frames)
    for f, s, res in blocks:
        out.append(T)
        T = same_pad(T, KT, s)[0]
    return out


class STGCNTA(STGCN):
    env_arithmetic = third_stream = False      # fp32, nothing to fork: no third stream (sar_amd/stgcn.py)

    def __init__(self, num_classes=60, in_channels=3, num_node=25, A=None, device="cuda", seed=0, bone_pairs=None, blocks=None,
                 motion=False, mfma="fp32", trainable_adjacency=True, frames=300):
        assert mfma == "fp32", "the per-frame adjacency engine is fp32"
        blocks = list(blocks) if blocks is not None else list(BLOCKS)
        self.frames = int(frames)
        self.block_T = block_frames(self.frames, blocks)
        self._tables_grad_dirty = True
        super().__init__(num_classes=num_classes, in_channels=in_channels, num_node=num_node, A=A, device=device, seed=seed,
                         bone_pairs=bone_pairs, blocks=blocks, motion=motion, mfma="fp32", trainable_adjacency=True)

    @staticmethod
    def table_name(i):
        return "l%d.adjacency_matrix" % i

    # ------------------------------------------------------------------ hooks of sar_amd/stgcn.py
    def _shared_adjacency(self):
        return False

    def _params_after_block(self, i):
        self._add(self.table_name(i), (KS, self.block_T[i], self.V, self.V))

    def _init_params(self, seed):
        """ST-GCN's initialisation; every table = the graph's adjacency repeated over the block's frames (stgcn_debug.py:129-132)"""
        super()._init_params(seed)
        self._repeat_adjacency(torch.from_numpy(self.A_host))

    def _repeat_adjacency(self, A, only=None):
        A = A.to(torch.float32).reshape(KS, 1, self.V, self.V)
        for i in range(len(self.blocks)):
            if only is None or i in only:
                self.p[self.table_name(i)].copy_(A.expand(KS, self.block_T[i], self.V, self.V))

    def _dense_fwd(self, i, y3, g, f, B, T, training):
        assert T == self.block_T[i]
        return ops.graph_dense_t_fwd(y3, self.p[self.table_name(i)], g, KS, f, self.V, B, T, stats=training)

    def _dense_bwd_data(self, i, dg, dy3, f, B, T):
        ops.graph_dense_t_bwd_data(dg, self.p[self.table_name(i)], dy3, KS, f, self.V, B, T)

    def _dense_dA(self, i, y3, dg, f, B, T):
        ops.graph_dense_t_dA(y3, dg, self.g[self.table_name(i)], KS, f, self.V, B, T)

    def _dense_backward_begin(self, dev):
        """trained: every block's backward overwrites its table gradient.  Frozen (main_gnn.py:228-232): no dadj launch, the table
        gradients are exactly zero -- zeroed once, they stay zero until the next trained step"""
        if self.train_adjacency:
            self._tables_grad_dirty = True
        elif self._tables_grad_dirty:
            for i in range(len(self.blocks)):
                self.g[self.table_name(i)].zero_()
            self._tables_grad_dirty = False

    def _dense_backward_end(self):
        pass

    # ------------------------------------------------------------------ forward / parameters
    def forward(self, x, training=True, keep=None):
        assert x.dim() == 5 and x.shape[2] == self.frames, \
            "this model owns one adjacency per frame: built for clips of %d frames, got %s" % (self.frames, tuple(x.shape))
        return super().forward(x, training=training, keep=keep)

    def load_params(self, params):
        """l{i}.adjacency_matrix as saved by state_dict; for a block without one, an ST-GCN dict's `A` (or `adjacency_matrix`) of shape
        (K, V, V) is repeated over the block's frames"""
        super().load_params(params)
        missing = [i for i in range(len(self.blocks)) if self.table_name(i) not in params]
        shared = params.get("adjacency_matrix", params.get("A"))
        if missing and shared is not None and tuple(shared.shape) == (KS, self.V, self.V):
            self._repeat_adjacency(shared.detach().cpu() if isinstance(shared, torch.Tensor) else torch.from_numpy(np.asarray(shared)),
                                   only=set(missing))
