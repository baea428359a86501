"""Shared helpers for the parity tests (layout conversion, error metrics)."""
import torch


def to_cn(x):
    """(B,C,T,V) -> CN matrix [C][B*T*V] (include/sar_hip.h)."""
    B, C, T, V = x.shape
    return x.permute(1, 0, 2, 3).reshape(C, B * T * V).contiguous()


def from_cn(y, B, T, V):
    C = y.shape[0]
    return y.reshape(C, B, T, V).permute(1, 0, 2, 3).contiguous()


def rel_err(a, b):
    """max |a-b| / max |b| (norm-wise relative error; b is the reference)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def rel_err_fro(a, b):
    """||a-b||_2 / ||b||_2 (Frobenius-relative error; b is the reference)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    denom = b.norm().item()
    return (a - b).norm().item() / (denom if denom > 0 else 1.0)


# ---- bf16 (CN8) kernels: exact definitions shared by tests/test_gpu_cn8.py and tests/test_gpu_cn8_batch64.py

def bf(t):
    """the value a bf16 operand holds (round to nearest even), as float64"""
    return t.float().bfloat16().double()


def assert_bf16_close(got, ref, what=""):
    """a stored bf16 output: within one bfloat16 rounding (2^-8 relative per element) plus 1e-5 of the tensor scale for the
    accumulation order"""
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().item()
    bad = (got - ref).abs() - (2.0 ** -8) * ref.abs() - 1e-5 * scale
    assert bad.max().item() <= 0, "%s: worst excess %.3e (scale %.3e)" % (what, bad.max().item(), scale)


def graph_ref(x, kernel, bias, A, dev_tables):
    """exact definition: z_k = bf16(fp32 gather of the bf16 src in table order), W rounded to bf16, float64 contraction"""
    idx, wt = dev_tables.idx.cpu(), dev_tables.wt.cpu()                   # [3][V][4]
    Bq, cin, T, V = x.shape
    f = kernel.shape[3] // 3
    xs = x.float()
    out = torch.zeros(Bq, f, T, V, dtype=torch.float64)
    Wk = bf(kernel)[0, 0]                                                  # (cin, 3f)
    for k in range(3):
        z = torch.zeros(Bq, cin, T, V)
        for w in range(V):
            acc = None
            for j in range(dev_tables.nz[k]):
                term = wt[k, w, j] * xs[:, :, :, idx[k, w, j]]
                acc = term if acc is None else torch.addcmul(acc, xs[:, :, :, idx[k, w, j]], wt[k, w, j])   # fp32 fma chain
            z[:, :, :, w] = acc
        zb = bf(z)
        out += torch.einsum("bctv,cm->bmtv", zb, Wk[:, k * f:(k + 1) * f])
        if bias is not None:
            out += bias.double()[k * f:(k + 1) * f].view(1, -1, 1, 1) * A[k].double().sum(dim=0).view(1, 1, 1, -1)
    return out
