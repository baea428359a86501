"""The adaptive adjacency of 2s-AGCN restated with a hand-written backward pass; runs in the dtype of its inputs (float64 is the oracle
of the AdaptiveAdjacency tests, float32 the band).

  theta = Conv1x1(K Ce, no bias)(x)      phi = Conv1x1(K Ce, bias)(x)          channel k Ce + e belongs to subset k
  S[n,k,v,w]     = (1 / (Ce T)) sum_{e,t} theta[n, k Ce + e, t, v] phi[n, k Ce + e, t, w]
  P[n,k,:,w]     = softmax over v of S[n,k,:,w]
  A_eff[n,k,v,w] = A[k,v,w] + P[n,k,v,w]

x (N, C, T, V), A (K, V, V), the kernels (C, K Ce) (the Keras (1, 1, C, K Ce) reshaped), phi_bias (K Ce)."""
import torch


def forward(x, A, theta_kernel, phi_kernel, phi_bias):
    """-> (A_eff (N, K, V, V), ctx)"""
    N, C, T, V = x.shape
    K = A.shape[0]
    tk, pk = theta_kernel.reshape(C, -1), phi_kernel.reshape(C, -1)
    Ce = tk.shape[1] // K
    theta = torch.einsum("nctv,cm->nmtv", x, tk)
    phi = torch.einsum("nctv,cm->nmtv", x, pk) + phi_bias.view(1, -1, 1, 1)
    th, ph = theta.reshape(N, K, Ce * T, V), phi.reshape(N, K, Ce * T, V)      # (e, t) is one index of stride V
    S = th.transpose(2, 3) @ ph / (Ce * T)
    e = torch.exp(S - S.max(dim=2, keepdim=True)[0])
    P = e / e.sum(dim=2, keepdim=True)
    ctx = dict(x=x, tk=tk, pk=pk, theta=theta, phi=phi, S=S, P=P, K=K, Ce=Ce)
    return A.unsqueeze(0) + P, ctx


def backward(ctx, dA_eff):
    """-> dict of dx, dtheta_kernel (C, K Ce), dphi_kernel (C, K Ce), dphi_bias (K Ce), dA (K, V, V) and the intermediates dS (N, K, V, V),
    dtheta / dphi (N, K Ce, T, V)"""
    x, tk, pk, P, K, Ce = ctx["x"], ctx["tk"], ctx["pk"], ctx["P"], ctx["K"], ctx["Ce"]
    N, C, T, V = x.shape
    g = (P * dA_eff).sum(dim=2, keepdim=True)
    dS = P * (dA_eff - g)
    th, ph = ctx["theta"].reshape(N, K, Ce * T, V), ctx["phi"].reshape(N, K, Ce * T, V)
    dtheta = (ph @ dS.transpose(2, 3) / (Ce * T)).reshape(N, K * Ce, T, V)      # [.., v] = sum_w dS[v, w] phi[.., w]
    dphi = (th @ dS / (Ce * T)).reshape(N, K * Ce, T, V)                        # [.., w] = sum_v dS[v, w] theta[.., v]
    dx = torch.einsum("nmtv,cm->nctv", dtheta, tk) + torch.einsum("nmtv,cm->nctv", dphi, pk)
    return dict(dx=dx, dtheta_kernel=torch.einsum("nctv,nmtv->cm", x, dtheta), dphi_kernel=torch.einsum("nctv,nmtv->cm", x, dphi),
                dphi_bias=dphi.sum(dim=(0, 2, 3)), dA=dA_eff.sum(dim=0), dS=dS, dtheta=dtheta, dphi=dphi)


def literal(x, A, theta_kernel, phi_kernel, phi_bias, theta_bias=None):
    """the formulation as 2s-AGCN writes it, one subset at a time, for torch autograd: conv -> permute / view -> matmul -> softmax(-2)"""
    N, C, T, V = x.shape
    K = A.shape[0]
    Ce = theta_kernel.reshape(C, -1).shape[1] // K
    conv = lambda kernel, bias: torch.nn.functional.conv2d(x, kernel.reshape(C, -1).t().reshape(-1, C, 1, 1), bias)
    theta, phi = conv(theta_kernel, theta_bias), conv(phi_kernel, phi_bias)
    out = []
    for k in range(K):
        a1 = theta[:, k * Ce:(k + 1) * Ce].permute(0, 3, 1, 2).reshape(N, V, Ce * T)
        a2 = phi[:, k * Ce:(k + 1) * Ce].reshape(N, Ce * T, V)
        out.append(A[k] + torch.softmax(torch.matmul(a1, a2) / (Ce * T), dim=-2))
    return torch.stack(out, dim=1)


def column_std(S):
    """the mean over the columns (n, k, w) of the standard deviation over v of the logits"""
    return S.std(dim=2, unbiased=False).mean().item()
