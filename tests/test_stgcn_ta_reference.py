"""tests/stgcn_ta_reference.py (the float64 restatement of models/stgcn_debug.py that the GPU tests of sar_amd/stgcn_ta.py compare
against) checked against oracle/stgcn.py and against finite differences.  CPU only."""
import numpy as np
import torch

from oracle import stgcn as O
import stgcn_ta_reference as R
from sar_amd.stgcn_ta import block_frames          # the engine's own frame counts (no GPU needed to import)
from util import rel_err

BLOCKS3 = [(64, 1, False), (64, 1, True), (128, 2, True)]


def _case(blocks, N, T, classes, seed):
    p = O.randomize_affine(O.init_params(classes, seed=seed, dtype=torch.float64, blocks=blocks), seed=seed + 1)
    x, y = O.synthetic_batch(N, seed=seed, T=T, num_classes=classes)
    return p, x.double(), y


def _reference_with_adjacency_leaf(p, x, y, blocks, masks=None):
    """oracle/stgcn.py's train step with the shared adjacency as one more differentiable leaf (as tests/test_gpu_adjacency.py)"""
    names = O.trainable_names(p) + ["A"]
    leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
    q = dict(p)
    q.update(leaves)
    logits = O.forward(q, x, True, {}, {}, blocks, masks)
    loss = O.loss_fn(logits, y, x.shape[0])
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return logits.detach(), loss.detach(), dict(zip(names, grads))


def test_repeated_adjacency_reproduces_the_oracle():
    """every table = A repeated over the frames: logits, loss, every shared gradient and the moving statistics are oracle.stgcn's;
    the table gradients summed over frames and blocks are the gradient of the shared A"""
    p, x, y = _case(BLOCKS3, 2, 14, 10, 0)
    logits0, loss0, grads0, stats0, _ = O.loss_and_grads(p, x, y, blocks=BLOCKS3)
    _, _, gleaf = _reference_with_adjacency_leaf(p, x, y, BLOCKS3)
    q = R.init_tables(dict(p), 14, BLOCKS3)
    logits, loss, grads, stats, _ = R.loss_and_grads(q, x, y, blocks=BLOCKS3)
    assert rel_err(logits, logits0) < 1e-12 and rel_err(loss.reshape(1), loss0.reshape(1)) < 1e-12
    for k, g in grads0.items():
        assert rel_err(grads[k], g) < 1e-12 or g.abs().max() < 1e-9 and (grads[k] - g).abs().max() < 1e-15, k
    for k, v in stats0.items():
        assert rel_err(stats[k], v) < 1e-12, k
    dA = sum(grads[R.table_name(i)].sum(dim=1) for i in range(len(BLOCKS3)))
    assert rel_err(dA, gleaf["A"]) < 1e-12
    assert set(grads) == set(grads0) | {R.table_name(i) for i in range(len(BLOCKS3))}


def test_table_gradient_against_central_differences():
    blocks = [(64, 1, False), (64, 1, True)]
    p, x, y = _case(blocks, 2, 12, 10, 3)
    q = R.init_tables(dict(p), 12, blocks)
    g = torch.Generator().manual_seed(9)
    for i in range(2):       # dense tables, different per frame
        q[R.table_name(i)] = q[R.table_name(i)] + 0.05 * torch.randn(q[R.table_name(i)].shape, generator=g, dtype=torch.float64)
    # (ReLU patterns fixed to those of the unperturbed point: the differences below stay on one linear piece)
    _, _, _, _, taps = R.loss_and_grads(q, x, y, blocks=blocks)
    masks = {}
    for i in range(2):
        pre = "l%d." % i
        bn = O.batch_norm(taps[pre + "g"], q[pre + "bn1.gamma"], q[pre + "bn1.beta"], None, None, True, (0, 2, 3), True)
        masks[pre + "h"], masks[pre + "y"] = bn > 0, taps[pre + "y"] > 0
    _, _, grads, _, _ = R.loss_and_grads(q, x, y, blocks=blocks, masks=masks)
    eps = 1e-5
    for i, idx in [(0, (0, 0, 0, 0)), (0, (1, 5, 3, 7)), (0, (2, 11, 24, 24)), (1, (0, 7, 20, 4)), (1, (2, 3, 12, 12)), (1, (1, 11, 0, 24))]:
        name = R.table_name(i)
        vals = []
        for sgn in (1.0, -1.0):
            qq = dict(q)
            qq[name] = q[name].clone()
            qq[name][idx] += sgn * eps
            vals.append(O.loss_fn(R.forward(qq, x, True, blocks=blocks, masks=masks), y, x.shape[0]).item())
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = grads[name][idx].item()
        scale = grads[name].abs().max().item()
        # central differences at eps = 1e-5 in float64: truncation ~eps^2, rounding ~1e-16 / eps -- both below 1e-9 absolute; a wrong
        # gradient is off by the order of `scale`
        assert abs(fd - an) < 1e-5 * scale + 1e-9, (name, idx, fd, an)


def test_initial_tables_and_frame_counts():
    from graph.ntu_rgb_d import Graph
    A = torch.from_numpy(np.asarray(Graph().A).astype(np.float32)).double()      # (the reference casts to float32: stgcn_debug.py:243)
    want = [300, 300, 300, 300, 300, 150, 150, 150, 75, 75]
    assert R.block_frames(300) == want and block_frames(300, O.BLOCKS) == want
    assert block_frames(20, BLOCKS3) == [20, 20, 20] and block_frames(13, [(64, 2, True), (64, 2, True), (64, 1, True)]) == [13, 7, 4]
    p = R.init_tables(O.init_params(60, seed=0, dtype=torch.float64), 300)
    for i, T in enumerate(want):
        tab = p[R.table_name(i)]
        assert tuple(tab.shape) == (3, T, 25, 25)
        assert all(torch.equal(tab[:, t], A) for t in (0, 1, T // 2, T - 1))
        assert torch.equal(tab, A.unsqueeze(1).expand(3, T, 25, 25))
