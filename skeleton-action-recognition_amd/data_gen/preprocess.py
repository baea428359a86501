"""data_gen/preprocess.py of the reference on the MI355X: `pre_normalization(data, zaxis, xaxis)` with the reference's signature,
computed by csrc/prenorm.hip (sar_amd.ops.pre_normalize) instead of Python loops over clips, bodies, frames and joints.

A CUDA tensor in gives a CUDA tensor out.  A numpy array (or memmap) in gives a numpy float32 array out: it crosses the device in
chunks of at most CHUNK clips through pinned staging buffers, so a whole data set (56 000 clips, 10 GB) needs 2 x CHUNK clips of
device memory.  Unlike the reference the input is not modified, and nothing is printed."""
import numpy as np

CHUNK = 1024   # clips per trip through the device (numpy input)


def pre_normalization(data, zaxis=[0, 1], xaxis=[8, 4]):
    import torch
    from sar_amd import ops
    if isinstance(data, torch.Tensor):
        if not data.is_cuda:
            raise TypeError("pre_normalization: a tensor must live on the GPU (pass host data as a numpy array)")
        return ops.pre_normalize(data.float().contiguous(), zaxis=zaxis, xaxis=xaxis)
    if data.ndim != 5 or data.shape[1] != 3:
        raise ValueError("pre_normalization: need (N, 3, T, V, M) coordinates, got %s" % (data.shape,))
    N = data.shape[0]
    out = np.empty(data.shape, np.float32)
    if N == 0:
        return out
    n = max(1, min(int(CHUNK), N))
    host_in = torch.empty((n,) + tuple(data.shape[1:]), dtype=torch.float32, pin_memory=True)
    host_out = torch.empty_like(host_in, pin_memory=True)
    dev_in = torch.empty(host_in.shape, dtype=torch.float32, device="cuda")
    dev_out = torch.empty_like(dev_in)
    for i in range(0, N, n):
        k = min(n, N - i)
        np.copyto(host_in.numpy()[:k], data[i:i + k], casting="same_kind")
        dev_in[:k].copy_(host_in[:k], non_blocking=True)
        ops.pre_normalize(dev_in[:k], dev_out[:k], zaxis=zaxis, xaxis=xaxis)
        host_out[:k].copy_(dev_out[:k], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out[i:i + k] = host_out.numpy()[:k]
    return out
