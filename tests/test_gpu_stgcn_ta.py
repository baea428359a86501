"""ST-GCN with a trainable adjacency per frame and per block (sar_amd/stgcn_ta.py, csrc/graph_dense_t.hip; the reference's
models/stgcn_debug.py): the three contraction kernels against a float64 einsum, the engine against the float64 restatement
tests/stgcn_ta_reference.py (conditioned on the engine's activation masks), the freeze switch, the gradient buckets, the drop-in
model and the CLI's --freeze-graph-until.  Tolerances are those of tests/test_gpu_adjacency.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import stgcn as O
import stgcn_ta_reference as R
from util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS3 = [(64, 1, False), (64, 1, True), (128, 2, True)]
K = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cn(x, ld=None):
    """(B, C, T, V) -> CN matrix [C][ld >= B*T*V]"""
    Bq, C, Tq, Vq = x.shape
    m = x.permute(1, 0, 2, 3).reshape(C, Bq * Tq * Vq)
    if ld is None:
        return m.contiguous()
    out = torch.full((C, ld), float("nan"))
    out[:, :m.shape[1]] = m
    return out


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("B,F,T,V", [(2, 64, 13, 25), (1, 20, 9, 25), (3, 128, 8, 25), (2, 16, 5, 18), (5, 256, 3, 25)])
def test_contraction_kernels_against_float64(dev, B, F, T, V):
    from sar_amd import ops
    g = torch.Generator().manual_seed(B * 100 + F)
    y = torch.randn(B, K * F, T, V, generator=g)
    At = torch.randn(K, T, V, V, generator=g) * 0.3
    dout = torch.randn(B, F, T, V, generator=g)
    addv = torch.randn(B, F, T, V, generator=g)
    yd = y.double().view(B, K, F, T, V).requires_grad_(True)
    Ad = At.double().requires_grad_(True)
    ref = torch.einsum("nkctv,ktvw->nctw", yd, Ad)
    gy, gA = torch.autograd.grad(ref, (yd, Ad), dout.double())
    n = B * T * V
    ld = n + 7                                        # leading dimension larger than B*T*V (the tail is NaN and must stay unread)
    yc, dc, ac, Ac = cn(y, ld).to(dev), cn(dout, ld).to(dev), cn(addv, ld).to(dev), At.to(dev).contiguous()
    out = torch.zeros((F, ld), device=dev)
    part, nparts = ops.graph_dense_t_fwd(yc, Ac, out, K, F, V, B, T, stats=True)
    out_add = torch.zeros((F, n), device=dev)
    part_add, _ = ops.graph_dense_t_fwd(yc, Ac, out_add, K, F, V, B, T, stats=True, add=ac)
    out_plain = torch.zeros((F, n), device=dev)
    assert ops.graph_dense_t_fwd(yc, Ac, out_plain, K, F, V, B, T) is None
    dy = torch.zeros((K * F, ld), device=dev)
    ops.graph_dense_t_bwd_data(dc, Ac, dy, K, F, V, B, T)
    dA = torch.empty((K, T, V, V), device=dev)
    ops.graph_dense_t_dA(yc, dc, dA, K, F, V, B, T)
    dA2 = torch.empty_like(dA)
    ops.graph_dense_t_dA(yc, dc, dA2, K, F, V, B, T)
    torch.cuda.synchronize()
    from sar_amd import _lib
    assert nparts == _lib.load().sar_graph_dense_t_nparts(B, T) and tuple(part.shape) == (F, nparts, 2)
    refc = cn(ref.detach())
    e_out, e_dy, e_dA = rel_err(out[:, :n].cpu(), refc), rel_err(dy[:, :n].cpu(), cn(gy.reshape(B, K * F, T, V))), rel_err(dA.cpu(), gA)
    p = part.cpu().double().sum(dim=1)
    e_p1, e_p2 = rel_err(p[:, 0], refc.sum(dim=1)), rel_err(p[:, 1], (refc * refc).sum(dim=1))
    refa = refc + cn(addv).double()
    pa = part_add.cpu().double().sum(dim=1)
    e_add, e_a1, e_a2 = rel_err(out_add.cpu(), refa), rel_err(pa[:, 0], refa.sum(dim=1)), rel_err(pa[:, 1], (refa * refa).sum(dim=1))
    print("out %.2e dy %.2e dAt %.2e sums %.2e %.2e | add: out %.2e sums %.2e %.2e" % (e_out, e_dy, e_dA, e_p1, e_p2, e_add, e_a1, e_a2))
    assert e_out < 2e-5 and e_dy < 2e-5 and e_dA < 2e-5
    assert e_p1 < 1e-4 and e_p2 < 2e-5
    assert e_add < 2e-5 and e_a1 < 1e-4 and e_a2 < 2e-5
    assert torch.equal(out_plain, out[:, :n])                  # statistics on / off: the same result
    assert (out[:, n:] == 0).all() and (dy[:, n:] == 0).all()  # nothing written past B*T*V
    assert torch.equal(dA, dA2)                                # repeated launches are bitwise equal


def _sample0(dev, B, F, T, V, y, dout, At):
    """out and dy of sample 0 from a launch over the first B samples"""
    from sar_amd import ops
    n = B * T * V
    yc, dc = cn(y[:B]).to(dev), cn(dout[:B]).to(dev)
    out, dy = torch.empty((F, n), device=dev), torch.empty((K * F, n), device=dev)
    ops.graph_dense_t_fwd(yc, At, out, K, F, V, B, T, stats=True)
    ops.graph_dense_t_bwd_data(dc, At, dy, K, F, V, B, T)
    torch.cuda.synchronize()
    return out[:, :T * V].clone(), dy[:, :T * V].clone()


def test_samples_are_independent_small(dev):
    g = torch.Generator().manual_seed(11)
    F, T, V = 48, 7, 25
    y, dout = torch.randn(5, K * F, T, V, generator=g), torch.randn(5, F, T, V, generator=g)
    At = (torch.randn(K, T, V, V, generator=g) * 0.3).to(dev)
    o2, d2 = _sample0(dev, 2, F, T, V, y, dout, At)
    o5, d5 = _sample0(dev, 5, F, T, V, y, dout, At)
    assert torch.equal(o2, o5) and torch.equal(d2, d5)


def test_samples_are_independent_at_the_bench_shape(dev):
    """B = 128, T = 300, F = 64 (bs = 64): sample 0 of the full launch is bitwise the single-sample launch"""
    from sar_amd import ops
    B, F, T, V = 128, 64, 300, 25
    g = torch.Generator(device=dev).manual_seed(12)
    n = B * T * V
    yc, dc = torch.randn((K * F, n), generator=g, device=dev), torch.randn((F, n), generator=g, device=dev)
    At = torch.randn((K, T, V, V), generator=g, device=dev) * 0.3
    out, dy = torch.empty((F, n), device=dev), torch.empty((K * F, n), device=dev)
    ops.graph_dense_t_fwd(yc, At, out, K, F, V, B, T, stats=True)
    ops.graph_dense_t_bwd_data(dc, At, dy, K, F, V, B, T)
    n1 = T * V
    out1, dy1 = torch.empty((F, n1), device=dev), torch.empty((K * F, n1), device=dev)
    ops.graph_dense_t_fwd(yc[:, :n1].contiguous(), At, out1, K, F, V, 1, T, stats=True)
    ops.graph_dense_t_bwd_data(dc[:, :n1].contiguous(), At, dy1, K, F, V, 1, T)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :n1], out1) and torch.equal(dy[:, :n1], dy1)
    ref = torch.einsum("kmtv,ktvw->mtw", yc[:, :n1].view(K, F, T, V).double(), At.double()).reshape(F, n1)
    assert rel_err(out1.cpu(), ref.cpu()) < 2e-5


# ------------------------------------------------------------------------------------------------ the engine
def _params(blocks, classes, seed):
    return O.randomize_affine(O.init_params(classes, seed=seed, dtype=torch.float64, blocks=blocks), seed=seed + 1)


def _perturbed_tables(p, frames, blocks, seed):
    """every entry of every table perturbed, differently per frame and per block"""
    R.init_tables(p, frames, blocks)
    g = torch.Generator().manual_seed(seed)
    for i in range(len(blocks)):
        k = R.table_name(i)
        p[k] = p[k] + 0.05 * torch.randn(p[k].shape, generator=g, dtype=torch.float64)
    return p


def test_repeated_adjacency_reproduces_stgcn(dev):
    from sar_amd.stgcn import STGCN
    from sar_amd.stgcn_ta import STGCNTA
    p = _params(BLOCKS3, 10, 2)
    x, y = O.synthetic_batch(3, seed=4, T=20, num_classes=10)
    fixed = STGCN(num_classes=10, device=dev, blocks=BLOCKS3, mfma="fp32")
    fixed.load_params(p)
    lf, _ = fixed.loss_and_grad(x.to(dev), y.to(dev))
    eng = STGCNTA(num_classes=10, device=dev, blocks=BLOCKS3, frames=20, seed=7)
    assert eng.block_T == [20, 20, 20]
    assert eng.n_params == fixed.n_params + sum(3 * T * 625 for T in eng.block_T)
    assert "adjacency_matrix" not in eng.shapes
    A32 = p["A"].float()
    for i in range(3):      # the initial value: Graph().A per frame
        assert torch.equal(eng.p[R.table_name(i)].cpu(), A32.unsqueeze(1).expand(3, 20, 25, 25))
    eng.load_params(p)      # an ST-GCN parameter dict: its A is repeated over the frames of every block
    for i in range(3):
        assert torch.equal(eng.p[R.table_name(i)].cpu(), A32.unsqueeze(1).expand(3, 20, 25, 25))
    le, _ = eng.loss_and_grad(x.to(dev), y.to(dev))
    torch.cuda.synchronize()
    assert rel_err(le.cpu(), lf.cpu()) < 1e-5
    worst = max((rel_err(eng.g[k].cpu(), fixed.g[k].cpu()), k) for k in fixed.g
                if fixed.g[k].abs().max() > 1e-9 and not k.endswith(("tcn.bias", "res.bias")))
    print("per-frame tables vs gather-list path, same adjacency: worst gradient difference %.2e (%s)" % worst)
    assert worst[0] < 1e-2


@pytest.fixture(scope="module")
def dense_case(dev):
    """one engine step with dense tables and its float64 reference (computed once, shared, not modified)"""
    from sar_amd.stgcn_ta import STGCNTA
    from test_gpu_stgcn_model import _engine_masks
    p = _perturbed_tables(_params(BLOCKS3, 10, 2), 20, BLOCKS3, 5)
    x, y = O.synthetic_batch(3, seed=4, T=20, num_classes=10)
    eng = STGCNTA(num_classes=10, device=dev, blocks=BLOCKS3, frames=20)
    eng.load_params(p)
    keep = {}
    eng.forward(x.to(dev), training=True, keep=keep)
    masks = _engine_masks(eng, keep, BLOCKS3, x.shape[0] * x.shape[4], x.shape[2])
    logits_ref, loss_ref, grads_ref, _, _ = R.loss_and_grads(p, x.double(), y, blocks=BLOCKS3, masks=masks)
    eng.load_params(p)
    logits, loss = eng.loss_and_grad(x.to(dev), y.to(dev))
    torch.cuda.synchronize()
    return dict(eng=eng, p=p, x=x, y=y, logits=logits.clone(), loss=loss.clone(), grad=eng.grad.clone(), logits_ref=logits_ref,
                loss_ref=loss_ref, grads_ref=grads_ref)


def test_dense_tables_match_the_float64_reference(dense_case):
    c = dense_case
    eng = c["eng"]
    assert rel_err(c["logits"].cpu(), c["logits_ref"]) < 1e-4 and rel_err(c["loss"].cpu(), c["loss_ref"].reshape(1)) < 1e-4
    flat = c["grad"]
    seen = 0
    for k, gref in c["grads_ref"].items():
        o = eng.offsets[k]
        got = flat[o:o + gref.numel()].view(gref.shape).cpu()
        if gref.abs().max() > 1e-9:
            e = rel_err(got, gref)
            if "adjacency_matrix" in k:
                print("%s %.2e" % (k, e))
                seen += 1
            assert e < 1e-4, k
    assert seen == 3


def test_frozen_tables(dense_case, dev):
    """train_adjacency = False: table gradients exactly zero, every other gradient bit-identical"""
    c = dense_case
    eng = c["eng"]
    eng.load_params(c["p"])
    eng.train_adjacency = False
    try:
        logits, _ = eng.loss_and_grad(c["x"].to(dev), c["y"].to(dev))
        eng.loss_and_grad(c["x"].to(dev), c["y"].to(dev))        # a second frozen step: still zero
        torch.cuda.synchronize()
    finally:
        eng.train_adjacency = True
    frozen = eng.grad.clone()
    tab = torch.zeros(frozen.numel(), dtype=torch.bool, device=dev)
    for i in range(3):
        k = R.table_name(i)
        o = eng.offsets[k]
        tab[o:o + eng.g[k].numel()] = True
        assert (eng.g[k] == 0).all() and c["grad"][o:o + eng.g[k].numel()].abs().max() > 0
    assert torch.equal(frozen[~tab], c["grad"][~tab])
    eng.load_params(c["p"])                                       # and trained again afterwards: the unfrozen step, bit for bit
    eng.loss_and_grad(c["x"].to(dev), c["y"].to(dev))
    torch.cuda.synchronize()
    assert torch.equal(eng.grad, c["grad"])


def test_clip_length_is_checked(dense_case, dev):
    x, _ = O.synthetic_batch(2, seed=1, T=16, num_classes=10)
    with pytest.raises(AssertionError, match="20 frames"):
        dense_case["eng"].forward(x.to(dev), training=False)


def test_full_model_is_finite_and_deterministic(dev):
    from sar_amd.stgcn import STGCN
    from sar_amd.stgcn_ta import STGCNTA
    from sar_amd.train import synthetic_clips
    x, y = synthetic_clips(2, dev, seed=3, num_classes=60)
    eng = STGCNTA(num_classes=60, device=dev, seed=0)
    assert eng.block_T == [300, 300, 300, 300, 300, 150, 150, 150, 75, 75]
    assert eng.n_params == STGCN(num_classes=60, device=dev, mfma="fp32").n_params + sum(3 * T * 625 for T in eng.block_T)
    state = {k: v.clone() for k, v in eng.state_dict().items()}
    ref = None
    for _ in range(2):
        eng.load_params(state)
        logits, loss = eng.loss_and_grad(x, y)
        torch.cuda.synchronize()
        cur = (logits.clone(), loss.clone(), eng.grad.clone())
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(ref, cur))
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[2]).all()
    assert all(eng.g[R.table_name(i)].abs().max().item() > 0 for i in range(10))


def test_sgd_training_steps_track_the_reference(dev):
    """three Nesterov steps against the float64 restatement; a parameter that misses 2e-4 is judged against eight times the
    distance of the float32 restatement (same steps, same activation patterns) from float64 (printed)"""
    from sar_amd.stgcn_ta import STGCNTA
    from test_gpu_stgcn_model import _engine_masks
    p = _perturbed_tables(_params(BLOCKS3, 10, 5), 20, BLOCKS3, 8)
    p32 = {k: v.float().clone() for k, v in p.items()}
    eng = STGCNTA(num_classes=10, device=dev, blocks=BLOCKS3, frames=20)
    eng.load_params(p)
    vel, vel32 = {}, {}
    for step in range(3):
        x, y = O.synthetic_batch(4, seed=10 + step, T=20, num_classes=10)
        stats = {n: (bn.moving_mean.clone(), bn.moving_var.clone()) for n, bn in eng.bn.items()}
        keep = {}
        eng.forward(x.to(dev), training=True, keep=keep)
        masks = _engine_masks(eng, keep, BLOCKS3, x.shape[0] * x.shape[4], x.shape[2])
        for n, (mm, mv) in stats.items():
            eng.bn[n].moving_mean.copy_(mm)
            eng.bn[n].moving_var.copy_(mv)
        lr = O.lr_schedule(step)
        _, loss_ref, grads, new, _ = R.loss_and_grads(p, x.double(), y, blocks=BLOCKS3, masks=masks)
        O.sgd_nesterov_step(p, grads, vel, lr)
        p.update(new)
        _, _, grads32, new32, _ = R.loss_and_grads(p32, x.float(), y, blocks=BLOCKS3, masks=masks)
        O.sgd_nesterov_step(p32, grads32, vel32, lr)
        p32.update(new32)
        _, loss = eng.loss_and_grad(x.to(dev), y.to(dev))
        eng.sgd_step(lr)
        torch.cuda.synchronize()
        assert rel_err(loss.cpu(), loss_ref.reshape(1)) < 1e-4
    sd = eng.state_dict()
    for k in [k for k in p if R.is_trainable(k)]:
        if k.endswith(("tcn.bias", "res.bias")):      # a bias in front of a train-mode BatchNorm
            assert (sd[k] - p[k].float()).abs().max().item() < 1e-5, k
            continue
        err, band = rel_err(sd[k], p[k]), rel_err(p32[k], p[k])
        if err >= 2e-4:
            print("%s: engine %.3e, float32 restatement %.3e from float64" % (k, err, band))
        assert err < max(2e-4, 8 * band), k


def test_inference_mode_and_state_dict_round_trip(dev):
    from sar_amd.stgcn_ta import STGCNTA
    p = _perturbed_tables(_params(BLOCKS3, 10, 6), 16, BLOCKS3, 9)
    x, _ = O.synthetic_batch(3, seed=3, T=16, num_classes=10)
    ref = torch.softmax(R.forward(p, x.double(), False, blocks=BLOCKS3), 1)
    eng = STGCNTA(num_classes=10, device=dev, blocks=BLOCKS3, frames=16)
    eng.load_params(p)
    probs = eng.predict(x.to(dev))
    torch.cuda.synchronize()
    assert rel_err(probs.cpu(), ref) < 1e-4
    sd = eng.state_dict()
    assert all(torch.equal(sd[R.table_name(i)], p[R.table_name(i)].float()) for i in range(3))
    other = STGCNTA(num_classes=10, device=dev, blocks=BLOCKS3, frames=16, seed=5)
    other.load_params(sd)        # (sd also holds the fixed 'A': the tables win)
    assert torch.equal(other.predict(x.to(dev)), probs)


def test_table_gradients_are_final_in_their_bucket(dev):
    """every slice handed to bucket_cb already holds its final value (the tables of its blocks included), and a bucketed run is
    bitwise the unbucketed run"""
    from sar_amd.stgcn_ta import STGCNTA
    blocks = [(64, 1, False), (64, 1, True), (128, 2, True), (128, 1, True), (256, 2, True)]
    p = _perturbed_tables(_params(blocks, 10, 3), 24, blocks, 4)
    x, y = O.synthetic_batch(2, seed=6, T=24, num_classes=10)
    eng = STGCNTA(num_classes=10, device=dev, blocks=blocks, frames=24)
    eng.load_params(p)
    eng.loss_and_grad(x.to(dev), y.to(dev))
    torch.cuda.synchronize()
    plain = eng.grad.clone()
    eng.grad.zero_()
    eng._tables_grad_dirty = True
    handed = []

    def cb(bi, flat, events):
        for ev in events:
            ev.synchronize()
        handed.append((bi, flat.clone()))

    eng.load_params(p)
    eng.loss_and_grad(x.to(dev), y.to(dev), bucket_cb=cb)
    torch.cuda.synchronize()
    assert [bi for bi, _ in handed] == list(range(len(eng._buckets))) and len(handed) == 3
    covered = set()
    for bi, got in handed:
        _, lo, hi = eng._buckets[bi]
        assert torch.equal(got, plain[lo:hi]), bi
        covered |= {i for i in range(len(blocks)) if lo <= eng.offsets[R.table_name(i)] < hi}
    assert covered == set(range(len(blocks)))
    assert torch.equal(eng.grad, plain)


# ------------------------------------------------------------------------------------------------ drop-in model and CLI
def test_dropin_model_autograd(dev):
    sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
    from models.stgcn_debug import Model
    model = Model(num_classes=60, device=dev, seed=1, frames=24, trainable_adjacency=False, stream="joint", mfma="fp32")
    names = [v.name for v in model.trainable_variables]
    assert sum("adjacency_matrix" in n for n in names) == 10 and len(model.adjacency_matrices) == 10
    assert tuple(model.adjacency_matrices[4].shape) == (3, 24, 25, 25) and tuple(model.adjacency_matrices[9].shape) == (3, 6, 25, 25)
    x, y = O.synthetic_batch(2, seed=1, T=24, num_classes=60)
    logits = model(x.to(dev), training=True)
    loss = torch.nn.functional.cross_entropy(logits, y.to(dev), reduction="sum") / 2
    loss.backward()
    auto = {k: getattr(model, k.replace(".", "_")).grad.clone() for k in model._names}
    lg, ls = model.engine.loss_and_grad(x.to(dev), y.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(lg, logits.detach()) and rel_err(loss.detach().cpu().reshape(1), ls.cpu()) < 1e-6
    gmax = max(model.engine.g[k].abs().max().item() for k in model._names)
    ratio = {k: (auto[k] - model.engine.g[k]).abs().max().item() / max(model.engine.g[k].abs().max().item(), 1e-2 * gmax)
             for k in model._names}
    print("autograd vs fused step, worst:", sorted(ratio.items(), key=lambda kv: -kv[1])[:5])
    assert max(ratio.values()) < 2e-4          # (as tests/test_gpu_stpgcn.py: dlogits from torch vs the fused softmax kernel)
    for i in range(10):
        k = "l%d.adjacency_matrix" % i
        assert auto[k].abs().max() > 0 and ratio[k] < 2e-4


def test_cli_freeze_graph_until(dev, tmp_path):
    """main_gnn.py --model stgcn_debug --freeze-graph-until 0: the tables are untouched after epoch 1 and trained in epoch 2;
    --resume from the last checkpoint runs"""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "skeleton-action-recognition_amd"))
    base = [sys.executable, os.path.join(ROOT, "skeleton-action-recognition_amd", "main_gnn.py"), "--model", "stgcn_debug", "--synthetic",
            "--synthetic-size", "16", "--batch-size", "4", "--max-iters", "2", "--save-freq", "1", "--freeze-graph-until", "0",
            "--log-dir", str(tmp_path)]
    out = subprocess.run(base + ["--num-epochs", "2"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    ck = sorted(glob.glob(os.path.join(str(tmp_path), "*", "checkpoints", "ckpt-*.pt")))
    assert len(ck) == 2
    from graph.ntu_rgb_d import Graph
    A0 = torch.from_numpy(Graph().A.astype(np.float32))
    m1, m2 = torch.load(ck[0])["model"], torch.load(ck[1])["model"]
    for i, T in enumerate([300, 300, 300, 300, 300, 150, 150, 150, 75, 75]):
        k = "l%d.adjacency_matrix" % i
        assert torch.equal(m1[k], A0.unsqueeze(1).expand(3, T, 25, 25)), k
        assert not torch.equal(m2[k], m1[k]) and torch.isfinite(m2[k]).all(), k
    out = subprocess.run(base + ["--num-epochs", "3", "--resume", ck[1]], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Resumed from" in out.stdout and "Epoch: 3" in out.stdout
    ck3 = glob.glob(os.path.join(str(tmp_path), "*", "checkpoints", "ckpt-3.pt"))
    assert len(ck3) == 1
    m3 = torch.load(ck3[0])["model"]
    assert all(torch.isfinite(v).all() for v in m3.values())
