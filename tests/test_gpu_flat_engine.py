"""The stream helpers of sar_amd/engine.py read self._side when they are called: bench.py sets `eng._side = None` on a live engine for
its isolated pass and puts the stream back afterwards.  An engine treated like that issues the same launches on the main stream --
its gradients are bit-identical with those of an untouched twin built with the same seed."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _stgcn(dev):
    from sar_amd.stgcn import STGCN
    from sar_amd.train import synthetic_clips
    x, y = synthetic_clips(2, dev, seed=11, num_classes=10, T=16)
    return (lambda: STGCN(num_classes=10, device=dev, blocks=[(64, 1, False), (64, 2, True)], seed=3)), x, y


def _resnet(dev):
    from sar_amd.resnet import ResNet18
    g = torch.Generator(device=dev).manual_seed(2)
    x, y = torch.randn((2, 1, 64, 64), generator=g, device=dev), torch.tensor([1, 3], device=dev)
    return (lambda: ResNet18(num_classes=10, num_filters=16, device=dev, seed=3)), x, y


@pytest.mark.parametrize("case", [_stgcn, _resnet])
def test_an_engine_without_its_side_stream_computes_the_same_gradients(dev, case):
    make, x, y = case(dev)
    twin, eng = make(), make()
    assert eng._side is not None and twin._side is not None
    twin.loss_and_grad(x, y)
    side, eng._side = eng._side, None
    eng.loss_and_grad(x, y)
    eng._side = side
    torch.cuda.synchronize()
    assert torch.isfinite(twin.grad).all() and twin.grad.abs().max().item() > 0
    assert torch.equal(eng.grad, twin.grad)
    for k in eng.shapes:
        assert torch.equal(eng.g[k], twin.g[k]), k
    # ... and with the stream back, the next step again
    twin.loss_and_grad(x, y)
    eng.loss_and_grad(x, y)
    torch.cuda.synchronize()
    assert torch.equal(eng.grad, twin.grad)
