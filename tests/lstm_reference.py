"""CPU restatement of the reference's models/lstm_sampler.py (TemporalSampler) from its semantics, in plain torch: the yardstick of
tests/test_gpu_lstm_sampler.py (run in float64 for the reference values and in float32 for the error bar), itself pinned against
torch.nn.LSTM and a hand-computed case by tests/test_lstm_reference.py.  Differentiable by torch autograd; works in the dtype of
its inputs.

Keras LSTM (TF2 defaults): gate order i, f, c, o along the 4u axis, activation tanh, recurrent activation sigmoid, with bias, zero
initial state, return_sequences=True.  params: a list of (kernel (F, 4u), recurrent_kernel (u, 4u), bias (4u)) per layer."""
import torch


def lstm_layer(x, kernel, recurrent_kernel, bias, return_state=False):
    """x (N, T, F) -> h (N, T, u) by an explicit step loop; return_state: also the post-activation gates (N, T, 4u) and c (N, T, u)"""
    N, T, _ = x.shape
    u = recurrent_kernel.shape[0]
    h, c = x.new_zeros(N, u), x.new_zeros(N, u)
    hs, gs, cs = [], [], []
    for t in range(T):
        z = x[:, t] @ kernel + h @ recurrent_kernel + bias
        i, f, o = torch.sigmoid(z[:, :u]), torch.sigmoid(z[:, u:2 * u]), torch.sigmoid(z[:, 3 * u:])
        g = torch.tanh(z[:, 2 * u:3 * u])
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h), gs.append(torch.cat([i, f, g, o], dim=1)), cs.append(c)
    if return_state:
        return torch.stack(hs, dim=1), torch.stack(gs, dim=1), torch.stack(cs, dim=1)
    return torch.stack(hs, dim=1)


def lstm_stack(x_lstm, params):
    """the Sequential of LSTM layers: x_lstm (N, T, F0) -> (N, T, u_last)"""
    h = x_lstm
    for kernel, recurrent_kernel, bias in params:
        h = lstm_layer(h, kernel, recurrent_kernel, bias)
    return h


def stable_topk(scores, k):
    """(values, indices) of the k largest per row, descending, equal scores in ascending index"""
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(scores, 1, order), order


def temporal_sampler(x, params, top_k, indices=None):
    """x (N, C, T, V) -> (out (N, C, top_k, V), scores (N, T), indices (N, top_k)).  The selection is `indices` when given, else the
    stable descending top-k of this function's own scores; the scale is always this function's scores at the selection."""
    N, C, T, V = x.shape
    xt = x.permute(0, 2, 3, 1)                                     # (N, T, V, C)
    scores = lstm_stack(xt.reshape(N, T, V * C), params)[:, :, 0]  # the last layer has one unit: always (N, T)
    if indices is None:
        indices = stable_topk(scores.detach(), top_k)[1]
    indices = indices.long()
    values = torch.gather(scores, 1, indices)
    picked = torch.gather(xt, 1, indices.view(N, top_k, 1, 1).expand(N, top_k, V, C))
    out = (picked * values.view(N, top_k, 1, 1)).permute(0, 3, 1, 2)
    return out, scores, indices
