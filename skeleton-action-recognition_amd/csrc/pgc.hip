// pgc.hip -- ProjectionGraphConv(64, 32) of ST-PGCN (models/stpgcn.py:11-47, its GraphConv models/gcn.py:22-37), fp32 CN layout.
// x is block 0's output [C = 64][B*P] (column b*P + p, P = T*V); J = 32 projection vertices; s = sigmoid(variance), r = 1/s.
//
//   assign      l[p,j] = -0.5 max(sum_c ((x[c,p] - centers[c,j]) r[c,j])^2, 1e-12); q = softmax_j(l) -> q [J][B*P];
//               the same pass writes per-workgroup partials of S = x q^T [C][J] and qs = sum_p q [J] (one column per lane, then
//               the workgroup's tile in LDS: each lane owns 16 (c, j) sums)
//   small fwd   one workgroup per sample: partials -> S, qs (fixed order); zp = (S - centers qs) / (s qs); zn = l2-normalised zp
//               over j; A = zn^T zn; g = W^T zn + bias; h = g A  -> saved [B][PGC_SAVED]
//   project     out[c,p] = x[c,p] + sum_j q[p,j] h[c,j]
//   bwd reduce  partials of dh = dout q^T per sample
//   small bwd   dh -> dg, dA, dW / dbias slabs, dzn, the l2-normalise backward, dS = dzp / (s qs), dqs, the pooled-path terms of
//               dcenters (-dzp / s) and ds (-dzp zp / s) per sample
//   bwd column  dq = dout^T h + x^T dS + dqs; dl = q (dq - sum_j q dq) (0 where the 1e-12 clamp holds);
//               dx = dout + dS q^T - sum_j dl z r; per-workgroup partials of sum_p dl z and sum_p dl z^2 (the logit-path dcenters / ds,
//               times r in the finalisation)
//   param grad  dcenters = pooled + r colsum, ds likewise, dvariance = ds s (1 - s)
// Every sum over columns is a per-workgroup partial reduced in a fixed order, and the partial count depends on P only (sar_pgc_nparts):
// no atomics, bitwise deterministic, and a sample's results do not depend on the other samples of the batch.
#include "sar_common.h"

namespace {

constexpr int PC = SAR_PGC_C, PJ = SAR_PGC_J;   // 64 channels, 32 vertices
constexpr int CJ = PC * PJ;                       // 2048
constexpr int TILE = 128;                         // columns per tile = lanes per workgroup of the column passes
constexpr int TPW = 4;                            // tiles per workgroup
constexpr int XS = TILE + 1;                      // LDS row stride of the x tile (conflict-free column writes, row reads)
constexpr int SMALL = 256;                        // lanes of the per-sample kernels
// saved[b] layout (floats)
constexpr int O_S = 0, O_ZP = CJ, O_ZN = 2 * CJ, O_G = 3 * CJ, O_H = 4 * CJ, O_A = 5 * CJ, O_QS = O_A + PJ * PJ, O_N2 = O_QS + PJ;
static_assert(O_N2 + PC == SAR_PGC_SAVED, "saved layout");
static_assert(CJ + PJ == SAR_PGC_FWD_PART && CJ == SAR_PGC_DH_PART && 2 * CJ == SAR_PGC_BWD_PART, "partial sizes");
static_assert(CJ + PJ == SAR_PGC_DSAVED && 2 * CJ + PC * PC + PC == SAR_PGC_SLAB, "slab sizes");

__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

// Phase 2 of the tile passes: lane t owns (c = t / 2, j = 16 (t % 2) .. + 16): acc[j] += sum_k xs[c][k] qs[k][j]
__device__ __forceinline__ void tile_outer(const float (*xs)[XS], const float (*qt)[PJ], int c, int j0, float (&acc)[16]) {
#pragma unroll 4
  for (int k = 0; k < TILE; ++k) {
    const float xv = xs[c][k];
    const float4* qr = reinterpret_cast<const float4*>(&qt[k][j0]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 v = qr[u];
      acc[4 * u + 0] = fmaf(xv, v.x, acc[4 * u + 0]);
      acc[4 * u + 1] = fmaf(xv, v.y, acc[4 * u + 1]);
      acc[4 * u + 2] = fmaf(xv, v.z, acc[4 * u + 2]);
      acc[4 * u + 3] = fmaf(xv, v.w, acc[4 * u + 3]);
    }
  }
}

// ASSIGN: q computed from x (and written), partials [S | qs]; else q read, partials dh = src q^T.  grid (nparts, B), TILE lanes.
template <bool ASSIGN>
__global__ __launch_bounds__(TILE) void pgc_tile_kernel(const float* __restrict__ src, int64_t ld_src, int64_t P,
                                                        const float* __restrict__ centers, const float* __restrict__ variance,
                                                        float* __restrict__ q, int64_t ld_q, float* __restrict__ part) {
  __shared__ float xs[PC][XS];
  __shared__ __attribute__((aligned(16))) float qt[TILE][PJ];
  __shared__ __attribute__((aligned(16))) float2 cr[ASSIGN ? CJ : 1];   // (centers, r)[c][j]
  const int t = threadIdx.x, g = blockIdx.x, b = blockIdx.y, G = gridDim.x;
  if (ASSIGN) {
    for (int e = t; e < CJ; e += TILE) cr[e] = make_float2(centers[e], 1.f / sigm(variance[e]));
    __syncthreads();
  }
  const int c2 = t >> 1, j0 = (t & 1) * 16;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float qsum = 0.f;
  const int64_t ntiles = (P + TILE - 1) / TILE;
  const int64_t t0 = (int64_t)g * TPW, t1 = t0 + TPW < ntiles ? t0 + TPW : ntiles;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t p = tile * TILE + t;
    const bool valid = p < P;
    const int64_t col = (int64_t)b * P + p;
    for (int c = 0; c < PC; ++c) xs[c][t] = valid ? src[(int64_t)c * ld_src + col] : 0.f;
    if (ASSIGN) {
      float d[PJ];
#pragma unroll
      for (int j = 0; j < PJ; ++j) d[j] = 0.f;
      for (int c = 0; c < PC; ++c) {
        const float xv = xs[c][t];
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
          const float2 w = cr[c * PJ + j];
          const float z = (xv - w.x) * w.y;
          d[j] = fmaf(z, z, d[j]);
        }
      }
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < PJ; ++j) {
        d[j] = -0.5f * fmaxf(d[j], 1e-12f);
        m = fmaxf(m, d[j]);
      }
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < PJ; ++j) {
        d[j] = expf(d[j] - m);
        sum += d[j];
      }
      const float inv = 1.f / sum;
#pragma unroll
      for (int j = 0; j < PJ; ++j) {
        const float qv = d[j] * inv;
        if (valid) q[(int64_t)j * ld_q + col] = qv;
        qt[t][j] = valid ? qv : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < PJ; ++j) qt[t][j] = valid ? q[(int64_t)j * ld_q + col] : 0.f;
    }
    __syncthreads();
    tile_outer(xs, qt, c2, j0, acc);
    if (ASSIGN && t < PJ)
      for (int k = 0; k < TILE; ++k) qsum += qt[k][t];
    __syncthreads();
  }
  const int E = ASSIGN ? CJ + PJ : CJ;
  float* out = part + ((int64_t)b * G + g) * E;
#pragma unroll
  for (int i = 0; i < 16; ++i) out[c2 * PJ + j0 + i] = acc[i];
  if (ASSIGN && t < PJ) out[CJ + t] = qsum;
}

// one workgroup per sample: the projected graph and its convolution
__global__ __launch_bounds__(SMALL) void pgc_small_fwd_kernel(const float* __restrict__ part, int nparts, const float* __restrict__ centers,
                                                              const float* __restrict__ variance, const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ saved) {
  __shared__ float S[CJ + PJ], zn[CJ], A[PJ * PJ], gg[CJ], n2s[PC];
  const int t = threadIdx.x, b = blockIdx.x;
  const float* pb = part + (int64_t)b * nparts * (CJ + PJ);
  float* sv = saved + (int64_t)b * SAR_PGC_SAVED;
  for (int e = t; e < CJ + PJ; e += SMALL) {
    float v = 0.f;
    for (int g = 0; g < nparts; ++g) v += pb[(int64_t)g * (CJ + PJ) + e];
    S[e] = v;
  }
  __syncthreads();
  const float* qs = S + CJ;
  for (int e = t; e < CJ; e += SMALL) {
    const int j = e & (PJ - 1);
    const float s = sigm(variance[e]);
    const float zp = (S[e] - centers[e] * qs[j]) / (s * qs[j]);
    zn[e] = zp;
    sv[O_S + e] = S[e];
    sv[O_ZP + e] = zp;
  }
  if (t < PJ) sv[O_QS + t] = qs[t];
  __syncthreads();
  if (t < PC) {                                   // tf.math.l2_normalize over the J axis
    float v = 0.f;
    for (int j = 0; j < PJ; ++j) v = fmaf(zn[t * PJ + j], zn[t * PJ + j], v);
    n2s[t] = v;
    sv[O_N2 + t] = v;
  }
  __syncthreads();
  for (int e = t; e < CJ; e += SMALL) {
    const float v = zn[e] / sqrtf(fmaxf(n2s[e / PJ], 1e-12f));
    zn[e] = v;
    sv[O_ZN + e] = v;
  }
  __syncthreads();
  for (int e = t; e < PJ * PJ; e += SMALL) {      // A = zn^T zn
    const int i = e / PJ, j = e & (PJ - 1);
    float v = 0.f;
    for (int c = 0; c < PC; ++c) v = fmaf(zn[c * PJ + i], zn[c * PJ + j], v);
    A[e] = v;
    sv[O_A + e] = v;
  }
  for (int e = t; e < CJ; e += SMALL) {           // Conv1D(64, 1): g[f][j] = sum_c W[0][c][f] zn[c][j] + bias[f]
    const int f = e / PJ, j = e & (PJ - 1);
    float v = 0.f;
    for (int c = 0; c < PC; ++c) v = fmaf(W[c * PC + f], zn[c * PJ + j], v);
    v += bias[f];
    gg[e] = v;
    sv[O_G + e] = v;
  }
  __syncthreads();
  for (int e = t; e < CJ; e += SMALL) {           // einsum('ncv,nvw->ncw', g, A)
    const int f = e / PJ, j = e & (PJ - 1);
    float v = 0.f;
    for (int i = 0; i < PJ; ++i) v = fmaf(gg[f * PJ + i], A[i * PJ + j], v);
    sv[O_H + e] = v;
  }
}

// out[c][col] = x[c][col] + sum_j q[j][col] h[b][c][j];  grid (ceil(P / 256), B)
__global__ __launch_bounds__(256) void pgc_project_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ q, int64_t ld_q,
                                                          const float* __restrict__ saved, int64_t P, float* __restrict__ out,
                                                          int64_t ld_out) {
  __shared__ __attribute__((aligned(16))) float h[CJ];
  const int b = blockIdx.y;
  const float* hb = saved + (int64_t)b * SAR_PGC_SAVED + O_H;
  for (int e = threadIdx.x; e < CJ; e += 256) h[e] = hb[e];
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int64_t col = (int64_t)b * P + p;
  float qv[PJ];
#pragma unroll
  for (int j = 0; j < PJ; ++j) qv[j] = q[(int64_t)j * ld_q + col];
  for (int c = 0; c < PC; ++c) {
    const float4* hr = reinterpret_cast<const float4*>(&h[c * PJ]);
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < PJ / 4; ++u) {
      const float4 v = hr[u];
      a = fmaf(qv[4 * u + 0], v.x, a);
      a = fmaf(qv[4 * u + 1], v.y, a);
      a = fmaf(qv[4 * u + 2], v.z, a);
      a = fmaf(qv[4 * u + 3], v.w, a);
    }
    out[(int64_t)c * ld_out + col] = x[(int64_t)c * ld_x + col] + a;
  }
}

// one workgroup per sample: backward of the projected graph convolution
__global__ __launch_bounds__(SMALL) void pgc_small_bwd_kernel(const float* __restrict__ part, int nparts, const float* __restrict__ variance,
                                                              const float* __restrict__ W, const float* __restrict__ saved,
                                                              float* __restrict__ dsaved, float* __restrict__ slab) {
  __shared__ float dh[CJ], dg[CJ], zn[CJ], dA[PJ * PJ], dzn[CJ], tmp[CJ], dot[PC];
  const int t = threadIdx.x, b = blockIdx.x;
  const float* pb = part + (int64_t)b * nparts * CJ;
  const float* sv = saved + (int64_t)b * SAR_PGC_SAVED;
  float* ds_out = dsaved + (int64_t)b * SAR_PGC_DSAVED;
  float* sl = slab + (int64_t)b * SAR_PGC_SLAB;
  for (int e = t; e < CJ; e += SMALL) {
    float v = 0.f;
    for (int g = 0; g < nparts; ++g) v += pb[(int64_t)g * CJ + e];
    dh[e] = v;
    zn[e] = sv[O_ZN + e];
  }
  __syncthreads();
  const float* A = sv + O_A;
  const float* gg = sv + O_G;
  for (int e = t; e < CJ; e += SMALL) {           // dg = dh A^T
    const int f = e / PJ, i = e & (PJ - 1);
    float v = 0.f;
    for (int j = 0; j < PJ; ++j) v = fmaf(dh[f * PJ + j], A[i * PJ + j], v);
    dg[e] = v;
  }
  for (int e = t; e < PJ * PJ; e += SMALL) {      // dA = g^T dh
    const int i = e / PJ, j = e & (PJ - 1);
    float v = 0.f;
    for (int f = 0; f < PC; ++f) v = fmaf(gg[f * PJ + i], dh[f * PJ + j], v);
    dA[e] = v;
  }
  __syncthreads();
  for (int e = t; e < PC * PC; e += SMALL) {      // dW[0][c][f] = sum_j zn[c][j] dg[f][j]
    const int c = e / PC, f = e & (PC - 1);
    float v = 0.f;
    for (int j = 0; j < PJ; ++j) v = fmaf(zn[c * PJ + j], dg[f * PJ + j], v);
    sl[e] = v;
  }
  if (t < PC) {
    float v = 0.f;
    for (int j = 0; j < PJ; ++j) v += dg[t * PJ + j];
    sl[PC * PC + t] = v;
  }
  for (int e = t; e < CJ; e += SMALL) {           // dzn = W dg + zn (dA + dA^T)
    const int c = e / PJ, j = e & (PJ - 1);
    float v = 0.f;
    for (int f = 0; f < PC; ++f) v = fmaf(W[c * PC + f], dg[f * PJ + j], v);
    for (int i = 0; i < PJ; ++i) v = fmaf(zn[c * PJ + i], dA[i * PJ + j] + dA[j * PJ + i], v);
    dzn[e] = v;
  }
  __syncthreads();
  if (t < PC) {
    float v = 0.f;
    for (int j = 0; j < PJ; ++j) v = fmaf(dzn[t * PJ + j], zn[t * PJ + j], v);
    dot[t] = v;
  }
  __syncthreads();
  const float* qs = sv + O_QS;
  float* pool = sl + PC * PC + PC;
  for (int e = t; e < CJ; e += SMALL) {
    const int c = e / PJ, j = e & (PJ - 1);
    const float n2 = sv[O_N2 + c], n = sqrtf(fmaxf(n2, 1e-12f));
    const float dzp = (n2 > 1e-12f ? dzn[e] - zn[e] * dot[c] : dzn[e]) / n;      // l2_normalize backward
    const float s = sigm(variance[e]), sq = s * qs[j];
    ds_out[e] = dzp / sq;                                                          // dS
    pool[e] = -dzp / s;                                                            // d centers, pooled path
    pool[CJ + e] = -dzp * sv[O_ZP + e] / s;                                        // d s, pooled path
    // two quotients, not dzp S / (s qs^2): for a vertex that takes almost no column (qs below 1e-19) s qs^2 is denormal or 0 in
    // float32 while dzp / (s qs) and S / qs -- a weighted mean of x -- are ordinary numbers
    tmp[e] = (-dzp / sq) * (sv[O_S + e] / qs[j]);
  }
  __syncthreads();
  if (t < PJ) {                                   // dqs[j] = -sum_c (dzp / (s qs)) (S / qs)
    float v = 0.f;
    for (int c = 0; c < PC; ++c) v += tmp[c * PJ + t];
    ds_out[CJ + t] = v;
  }
}

// the fused backward column pass: dq, the softmax backward, dx; partials of sum_p dl z and sum_p dl z^2.  grid (nparts, B), TILE lanes.
__global__ __launch_bounds__(TILE) void pgc_bwd_column_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ dout,
                                                              int64_t ld_dout, const float* __restrict__ q, int64_t ld_q,
                                                              const float* __restrict__ saved, const float* __restrict__ dsaved,
                                                              const float* __restrict__ centers, const float* __restrict__ variance,
                                                              int64_t P, float* __restrict__ dx, int64_t ld_dx, float* __restrict__ part) {
  __shared__ float xs[PC][XS];
  __shared__ __attribute__((aligned(16))) float dlt[TILE][PJ];
  __shared__ __attribute__((aligned(16))) float4 prm[CJ];        // (centers, r, h, dS)[c][j]
  __shared__ float dqs[PJ];
  const int t = threadIdx.x, g = blockIdx.x, b = blockIdx.y, G = gridDim.x;
  const float* sv = saved + (int64_t)b * SAR_PGC_SAVED;
  const float* dsv = dsaved + (int64_t)b * SAR_PGC_DSAVED;
  for (int e = t; e < CJ; e += TILE) prm[e] = make_float4(centers[e], 1.f / sigm(variance[e]), sv[O_H + e], dsv[e]);
  if (t < PJ) dqs[t] = dsv[CJ + t];
  const int c2 = t >> 1, j0 = (t & 1) * 16;
  float cen[16], rr[16], accC[16], accS[16];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float4 w = prm[c2 * PJ + j0 + i];
    cen[i] = w.x;
    rr[i] = w.y;
    accC[i] = accS[i] = 0.f;
  }
  const int64_t ntiles = (P + TILE - 1) / TILE;
  const int64_t t0 = (int64_t)g * TPW, t1 = t0 + TPW < ntiles ? t0 + TPW : ntiles;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t p = tile * TILE + t;
    const bool valid = p < P;
    const int64_t col = (int64_t)b * P + p;
    for (int c = 0; c < PC; ++c) xs[c][t] = valid ? x[(int64_t)c * ld_x + col] : 0.f;
    float d[PJ], dq[PJ], qv[PJ];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      d[j] = 0.f;
      dq[j] = 0.f;
      qv[j] = valid ? q[(int64_t)j * ld_q + col] : 0.f;
    }
    for (int c = 0; c < PC; ++c) {
      const float xv = xs[c][t];
      const float dv = valid ? dout[(int64_t)c * ld_dout + col] : 0.f;
#pragma unroll
      for (int j = 0; j < PJ; ++j) {
        const float4 w = prm[c * PJ + j];
        const float z = (xv - w.x) * w.y;
        d[j] = fmaf(z, z, d[j]);
        dq[j] = fmaf(dv, w.z, dq[j]);
        dq[j] = fmaf(xv, w.w, dq[j]);
      }
    }
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      dq[j] += dqs[j];
      sq = fmaf(qv[j], dq[j], sq);
    }
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      dq[j] = d[j] > 1e-12f ? qv[j] * (dq[j] - sq) : 0.f;       // dl (softmax backward; the clamp passes no gradient)
      dlt[t][j] = dq[j];
    }
    for (int c = 0; c < PC; ++c) {
      const float xv = xs[c][t];
      float a = valid ? dout[(int64_t)c * ld_dout + col] : 0.f;
#pragma unroll
      for (int j = 0; j < PJ; ++j) {
        const float4 w = prm[c * PJ + j];
        const float z = (xv - w.x) * w.y;
        a = fmaf(qv[j], w.w, a);
        a = fmaf(-dq[j] * z, w.y, a);
      }
      if (valid) dx[(int64_t)c * ld_dx + col] = a;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < TILE; ++k) {
      const float xv = xs[c2][k];
      const float4* lr = reinterpret_cast<const float4*>(&dlt[k][j0]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 v = lr[u];
        const float dl4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int i = 4 * u + w;
          const float z = (xv - cen[i]) * rr[i];
          const float tz = dl4[w] * z;
          accC[i] += tz;
          accS[i] = fmaf(tz, z, accS[i]);
        }
      }
    }
    __syncthreads();
  }
  float* out = part + ((int64_t)b * G + g) * (2 * CJ);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    out[c2 * PJ + j0 + i] = accC[i];
    out[CJ + c2 * PJ + j0 + i] = accS[i];
  }
}

// dcenters = pooled + r colsum, ds = pooled + r colsum, dvariance = ds s (1 - s)
__global__ __launch_bounds__(256) void pgc_param_grad_kernel(const float* __restrict__ colsum, const float* __restrict__ pooled,
                                                             const float* __restrict__ variance, float* __restrict__ dcenters,
                                                             float* __restrict__ dvariance) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= CJ) return;
  const float s = sigm(variance[e]), r = 1.f / s;
  dcenters[e] = pooled[e] + r * colsum[e];
  const float ds = pooled[CJ + e] + r * colsum[CJ + e];
  dvariance[e] = ds * s * (1.f - s);
}

int tile_check(const char* what, const void* a, const void* b, int B, int64_t P, int64_t ld, const void* part) {
  SAR_REQUIRE(a && b && part && B >= 1 && P >= 1 && ld >= (int64_t)B * P, "%s: bad arguments", what);
  SAR_REQUIRE((P + TILE - 1) / TILE <= (int64_t)TPW * 65535 && B <= 65535, "%s: too large", what);
  return 0;
}

}  // namespace

extern "C" int sar_pgc_nparts(int64_t P) {
  if (P < 1) return 0;
  return (int)(((P + TILE - 1) / TILE + TPW - 1) / TPW);
}

extern "C" int sar_pgc_assign_f32(const float* x, int64_t ld_x, int B, int64_t P, const float* centers, const float* variance, float* q,
                                  float* part, sar_stream_t s) {
  if (int rc = tile_check("sar_pgc_assign", x, q, B, P, ld_x, part)) return rc;
  SAR_REQUIRE(centers && variance, "sar_pgc_assign: bad arguments");
  hipLaunchKernelGGL(pgc_tile_kernel<true>, dim3(sar_pgc_nparts(P), B), dim3(TILE), 0, as_stream(s), x, ld_x, P, centers, variance, q,
                     (int64_t)B * P, part);
  SAR_LAUNCH_CHECK("sar_pgc_assign_f32");
  return 0;
}

extern "C" int sar_pgc_small_fwd_f32(const float* part, int B, int nparts, const float* centers, const float* variance, const float* W,
                                     const float* bias, float* saved, sar_stream_t s) {
  SAR_REQUIRE(part && centers && variance && W && bias && saved && B >= 1 && B <= 65535 && nparts >= 1,
              "sar_pgc_small_fwd: bad arguments");
  hipLaunchKernelGGL(pgc_small_fwd_kernel, dim3(B), dim3(SMALL), 0, as_stream(s), part, nparts, centers, variance, W, bias, saved);
  SAR_LAUNCH_CHECK("sar_pgc_small_fwd_f32");
  return 0;
}

extern "C" int sar_pgc_project_f32(const float* x, int64_t ld_x, const float* q, const float* saved, int B, int64_t P, float* out,
                                   int64_t ld_out, sar_stream_t s) {
  SAR_REQUIRE(x && q && saved && out && B >= 1 && B <= 65535 && P >= 1 && ld_x >= (int64_t)B * P && ld_out >= (int64_t)B * P &&
              (P + 255) / 256 < (1ll << 31), "sar_pgc_project: bad arguments");
  hipLaunchKernelGGL(pgc_project_kernel, dim3((unsigned)((P + 255) / 256), B), dim3(256), 0, as_stream(s), x, ld_x, q, (int64_t)B * P,
                     saved, P, out, ld_out);
  SAR_LAUNCH_CHECK("sar_pgc_project_f32");
  return 0;
}

extern "C" int sar_pgc_bwd_reduce_f32(const float* dout, int64_t ld_dout, const float* q, int B, int64_t P, float* part, sar_stream_t s) {
  if (int rc = tile_check("sar_pgc_bwd_reduce", dout, q, B, P, ld_dout, part)) return rc;
  hipLaunchKernelGGL(pgc_tile_kernel<false>, dim3(sar_pgc_nparts(P), B), dim3(TILE), 0, as_stream(s), dout, ld_dout, P,
                     (const float*)nullptr, (const float*)nullptr, const_cast<float*>(q), (int64_t)B * P, part);
  SAR_LAUNCH_CHECK("sar_pgc_bwd_reduce_f32");
  return 0;
}

extern "C" int sar_pgc_small_bwd_f32(const float* part, int B, int nparts, const float* variance, const float* W, const float* saved,
                                     float* dsaved, float* slab, sar_stream_t s) {
  SAR_REQUIRE(part && variance && W && saved && dsaved && slab && B >= 1 && B <= 65535 && nparts >= 1, "sar_pgc_small_bwd: bad arguments");
  hipLaunchKernelGGL(pgc_small_bwd_kernel, dim3(B), dim3(SMALL), 0, as_stream(s), part, nparts, variance, W, saved, dsaved, slab);
  SAR_LAUNCH_CHECK("sar_pgc_small_bwd_f32");
  return 0;
}

extern "C" int sar_pgc_bwd_column_f32(const float* x, int64_t ld_x, const float* dout, int64_t ld_dout, const float* q, const float* saved,
                                      const float* dsaved, const float* centers, const float* variance, int B, int64_t P, float* dx,
                                      int64_t ld_dx, float* part, sar_stream_t s) {
  if (int rc = tile_check("sar_pgc_bwd_column", x, q, B, P, ld_x, part)) return rc;
  SAR_REQUIRE(dout && saved && dsaved && centers && variance && dx && ld_dout >= (int64_t)B * P && ld_dx >= (int64_t)B * P,
              "sar_pgc_bwd_column: bad arguments");
  hipLaunchKernelGGL(pgc_bwd_column_kernel, dim3(sar_pgc_nparts(P), B), dim3(TILE), 0, as_stream(s), x, ld_x, dout, ld_dout, q,
                     (int64_t)B * P, saved, dsaved, centers, variance, P, dx, ld_dx, part);
  SAR_LAUNCH_CHECK("sar_pgc_bwd_column_f32");
  return 0;
}

extern "C" int sar_pgc_param_grad_f32(const float* colsum, const float* pooled, const float* variance, float* dcenters, float* dvariance,
                                      sar_stream_t s) {
  SAR_REQUIRE(colsum && pooled && variance && dcenters && dvariance, "sar_pgc_param_grad: bad arguments");
  hipLaunchKernelGGL(pgc_param_grad_kernel, dim3(CJ / 256), dim3(256), 0, as_stream(s), colsum, pooled, variance, dcenters, dvariance);
  SAR_LAUNCH_CHECK("sar_pgc_param_grad_f32");
  return 0;
}
