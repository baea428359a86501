"""ST-PGCN training engine: the reference's extension of ST-GCN (models/stpgcn.py) on the HIP kernels.  The network is ST-GCN's
(same 10 blocks, data_bn prologue and head: sar_amd/stgcn.py) with ProjectionGraphConv(64, 32) between block 0 and block 1
(models/stpgcn.py:141-152; the layer :11-47, its GraphConv models/gcn.py:22-37):

    q   = softmax_j(-0.5 max(sum_c ((x - centers) / sigmoid(variance))^2, 1e-12))    x: block 0's output, per column
    zp  = (x q^T - centers qs) / (s qs);  zn = l2_normalize_j(zp);  A = zn^T zn          per sample, [64][32] / [32][32]
    out = x + q (Conv1D(64, 1)(zn) A)^T

on csrc/pgc.hip (sar_amd/ops.py: pgc_forward / pgc_backward).  The layer's parameters sit between l0.* and l1.* in the flat buffer,
so that their gradient falls in the last gradient bucket (handed to the all-reduce at the end of backward, after this layer's
backward has run).  fp32 only, fixed adjacency.
"""
import math

import torch

from . import ops
from .stgcn import STGCN

PGC_AFTER = 0            # the layer follows block 0 (models/stpgcn.py:142-143)
PGC_VERTICES = 32


def glorot_uniform(shape, gen):
    """Keras' default initializer of add_weight: U(-l, l), l = sqrt(6 / (fan_in + fan_out)), receptive field = prod(shape[:-2]);
    for (1, 64, 1, 32): fan_in = 64, fan_out = 2 048, l = 0.0533"""
    rf = int(math.prod(shape[:-2]))
    limit = math.sqrt(6.0 / (shape[-2] * rf + shape[-1] * rf))
    return (torch.rand(shape, dtype=torch.float64, generator=gen) * 2 - 1) * limit


class STPGCN(STGCN):
    env_arithmetic = third_stream = False      # fp32, nothing to fork: no third stream (sar_amd/stgcn.py)

    def __init__(self, num_classes=60, in_channels=3, num_node=25, A=None, device="cuda", seed=0, bone_pairs=None, blocks=None,
                 motion=False, mfma="fp32", trainable_adjacency=False):
        assert mfma == "fp32", "the ST-PGCN engine is fp32"
        assert not trainable_adjacency, "the ST-PGCN engine keeps the adjacency fixed"
        blocks = list(blocks) if blocks is not None else None
        super().__init__(num_classes=num_classes, in_channels=in_channels, num_node=num_node, A=A, device=device, seed=seed,
                         bone_pairs=bone_pairs, blocks=blocks, motion=motion, mfma="fp32", trainable_adjacency=False)

    # ------------------------------------------------------------------ hooks of sar_amd/stgcn.py
    def _params_after_block(self, i):
        if i != PGC_AFTER:
            return
        f = self.blocks[i][0]
        assert f == ops.PGC_C, "ProjectionGraphConv(64, 32) needs 64 channels out of block %d" % i
        J = PGC_VERTICES
        self._add("pgc.centers", (1, f, 1, J)), self._add("pgc.variance", (1, f, 1, J))
        self._add("pgc.gcn.kernel", (1, f, f)), self._add("pgc.gcn.bias", (f,))      # Conv1D(filters = 64, 1) in Keras layout

    def _layer_after(self, i):
        return i == PGC_AFTER

    def _init_params(self, seed):
        """ST-GCN's initialisation (the Conv1D kernel included: VarianceScaling(2, fan_out = 64, truncated normal), bias 0), then
        centers and variance from add_weight's default glorot_uniform: fan_in = 64, fan_out = 32 * 64 (models/stpgcn.py:18-21)"""
        super()._init_params(seed)
        gen = torch.Generator().manual_seed(seed + 104729)
        for k in ("pgc.centers", "pgc.variance"):
            self.p[k].copy_(glorot_uniform(self.shapes[k], gen).to(torch.float32))

    def _after_block_forward(self, i, h, B, T, training, saved, keep):
        if i != PGC_AFTER:
            return h
        P = T * self.V
        out = torch.empty_like(h)
        q, sv = ops.pgc_forward(h, B, P, self.p["pgc.centers"], self.p["pgc.variance"], self.p["pgc.gcn.kernel"],
                                self.p["pgc.gcn.bias"], out)
        if training:
            saved["pgc"] = dict(x=h, q=q, saved=sv, P=P)
        if keep is not None:
            J, C = PGC_VERTICES, ops.PGC_C
            keep["pgc.q"], keep["pgc.out"] = q, out
            keep["pgc.zn"] = sv[:, 2 * C * J:3 * C * J].view(B, C, J)
            keep["pgc.A"] = sv[:, 5 * C * J:5 * C * J + J * J].view(B, J, J)
        return out

    def _after_block_backward(self, i, dY, B):
        if i != PGC_AFTER:
            return dY
        s = self._saved["pgc"]
        dx = torch.empty_like(dY)
        o = self.offsets["pgc.gcn.kernel"]
        ops.pgc_backward(s["x"], dY, s["q"], s["saved"], B, s["P"], self.p["pgc.centers"], self.p["pgc.variance"],
                         self.p["pgc.gcn.kernel"], dx, self.g["pgc.centers"], self.g["pgc.variance"],
                         self.grad[o:o + ops.PGC_C * ops.PGC_C + ops.PGC_C])
        return dx
