// pgpool.hip -- ProjectionGraphPool(J) of ST-PGCNP (models/stpgcnp.py:11-38), fp32, any 1 <= C <= 512 channels, 1 <= J <= 512 vertices,
// P >= 1 columns per sample.  x is a CN matrix [C][ld >= B*P] (column b*P + p); tab = [r | r^2 | r^2 centers | s] ([C][J] each),
// s = sigmoid(variance), r = 1 / s.  Per-sample tensors ([B][C][J], [B][J][J], [B][J], [B][C]) are contiguous.
//
//   prep          tab from centers / variance
//   assign        d[p,j] = sum_c ((x[c,p] - centers[c,j]) r[c,j])^2 in DIFFERENCE form on the VALU: fp32 over blocks of 16 channels,
//                 the blocks added in fp64 (the logits are ~ -250 and differ by ~ 0.5 between vertices at the reference's
//                 initialisation: an fp32 running sum loses what the softmax needs); l = -0.5 max(d, 1e-12) minus the column's
//                 l[p,0] in fp64, only then rounded; q = softmax_j(l) -> q [J][ld_q]; one bit per (p, j) where the clamp held
//   moment        out[b] = x_b^(1|2) w_b^T ([C][J]; w = q: S; w = dl: the logit-path sums of the parameter gradients)      MFMA
//   rowsum        out[b][j] = sum_p w[j, (b, p)]
//   normalize     zp = (S - centers qs) / (s qs) (over S), n2 = sum_j zp^2, zn = zp / sqrt(max(n2, 1e-12))
//   gram          A_out[b] = zn_b^T zn_b                                                                                   MFMA
//   gram_bwd      dzn = dz + zn (dA + dA^T)                                                                                MFMA
//   normalize_bwd dS = dzp / (s qs) with dzp the l2-normalise backward of dzn; dqs[b][j] = -sum_c dS (zp s + centers)
//   dq            dq[j, (b, p)] = sum_c dS[b][c][j] x[c, (b, p)] + dqs[b][j]                                                 MFMA
//   softmax_bwd   dl = q (dq - sum_j q dq), 0 where the clamp held (in place over dq)
//   dx            dx = dS q - x * (r^2 dl) + (r^2 centers) dl  -- sum_j dl r^2 (x - centers) split into its two products   MFMA
//   param_grad    dcenters = sum_b [r^2 (M1 - centers M0) - dS qs], ds = sum_b [r^3 (M2 - 2 centers M1 + centers^2 M0) - dS qs zp],
//                 dvariance = ds s (1 - s); M0 = rowsum(dl), M1 = moment(x, dl), M2 = moment(x^2, dl); the sum over b in fp64
// No tensor with both a P and a C x J extent is written.  Every product is one workgroup tile that walks its whole contraction
// axis in a fixed order (no split, no atomics; one partial whatever P is); sums over lanes are xor trees: bitwise deterministic,
// and every kernel's grid has the sample as its own axis, so a sample's results do not depend on the rest of the batch.
// A vertex with qs == 0 gives 0 / 0 as in the reference (no guard).
#include "sar_common.h"

namespace {

constexpr int MAXD = SAR_PGPOOL_MAX;             // 512: C and J
constexpr float EPS = 1e-12f;

__device__ __forceinline__ float wave_max(float x) {
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m));
  return x;
}

// the same total in every lane of a 256-lane workgroup: xor tree per wave, the four waves in order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void pgpool_prep_kernel(const float* __restrict__ centers, const float* __restrict__ variance, int n,
                                                          float* __restrict__ tab) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float s = 1.f / (1.f + expf(-variance[e])), r = 1.f / s, r2 = r * r;
  tab[e] = r;
  tab[n + e] = r2;
  tab[2 * n + e] = r2 * centers[e];
  tab[3 * n + e] = s;
}

// ---- assign: grid (ceil(P / ATP), B), 256 lanes; lane t owns the vertices t (and t + 256: NJ = 2) for all ATP columns of the tile
constexpr int ATP = 16, ACH = 64, ASUB = 16, ALS = MAXD + 4;

template <int NJ>
__global__ __launch_bounds__(256) void pgpool_assign_kernel(const float* __restrict__ x, int64_t ld_x, int P, int C, int J,
                                                            const float* __restrict__ centers, const float* __restrict__ rtab,
                                                            float* __restrict__ q, int64_t ld_q, uint32_t* __restrict__ clamp, int W) {
  __shared__ __attribute__((aligned(16))) float xs[ACH][ATP];
  __shared__ float lt[ATP][ALS];
  __shared__ double lref[ATP];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.y;
  const int p0 = blockIdx.x * ATP;
  const int64_t col0 = (int64_t)b * P + p0;
  float acc[NJ][ATP];
  double tot[NJ][ATP];
#pragma unroll
  for (int u = 0; u < NJ; ++u)
#pragma unroll
    for (int p = 0; p < ATP; ++p) tot[u][p] = 0.0;
  for (int c0 = 0; c0 < C; c0 += ACH) {
    __syncthreads();                               // the previous chunk has been read
#pragma unroll
    for (int i = 0; i < ACH * ATP / 256; ++i) {
      const int cc = (t >> 4) + 16 * i, p = t & 15, c = c0 + cc;
      xs[cc][p] = (c < C && p0 + p < P) ? x[(int64_t)c * ld_x + col0 + p] : 0.f;
    }
    __syncthreads();
    for (int sub = 0; sub < ACH && c0 + sub < C; sub += ASUB) {
#pragma unroll
      for (int u = 0; u < NJ; ++u)
#pragma unroll
        for (int p = 0; p < ATP; ++p) acc[u][p] = 0.f;
#pragma unroll 4
      for (int ci = 0; ci < ASUB; ++ci) {
        const int c = c0 + sub + ci;
        float cv[NJ], rv[NJ];
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
          const int j = t + 256 * u;
          const bool ok = c < C && j < J;          // (a channel or vertex that does not exist: z = 0)
          cv[u] = ok ? centers[c * J + j] : 0.f;
          rv[u] = ok ? rtab[c * J + j] : 0.f;
        }
        float xv[ATP];
        const float4* xr = reinterpret_cast<const float4*>(&xs[sub + ci][0]);
#pragma unroll
        for (int k = 0; k < ATP / 4; ++k) {
          const float4 v = xr[k];
          xv[4 * k] = v.x, xv[4 * k + 1] = v.y, xv[4 * k + 2] = v.z, xv[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int u = 0; u < NJ; ++u)
#pragma unroll
          for (int p = 0; p < ATP; ++p) {
            const float z = (xv[p] - cv[u]) * rv[u];
            acc[u][p] = fmaf(z, z, acc[u][p]);
          }
      }
#pragma unroll
      for (int u = 0; u < NJ; ++u)
#pragma unroll
        for (int p = 0; p < ATP; ++p) tot[u][p] += (double)acc[u][p];
    }
  }
  // the clamp bits (wave w holds the vertices 64 (w + 4 u) .. + 63) and the logits
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = t + 256 * u, k = w + 4 * u;
#pragma unroll
    for (int p = 0; p < ATP; ++p) {
      const bool held = j < J && tot[u][p] <= (double)EPS;
      const unsigned long long bits = __ballot(held);
      if (lane == 0 && 64 * k < J && p0 + p < P) {
        clamp[(col0 + p) * W + 2 * k] = (uint32_t)bits;
        clamp[(col0 + p) * W + 2 * k + 1] = (uint32_t)(bits >> 32);
      }
      tot[u][p] = -0.5 * fmax(tot[u][p], (double)EPS);
    }
  }
  if (t == 0)
#pragma unroll
    for (int p = 0; p < ATP; ++p) lref[p] = tot[0][p];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = t + 256 * u;
    if (j < J)
#pragma unroll
      for (int p = 0; p < ATP; ++p) lt[p][j] = (float)(tot[u][p] - lref[p]);
  }
  __syncthreads();
  for (int p = w; p < ATP; p += 4) {               // softmax of one column per wave
    float v[MAXD / 64], m = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXD / 64; ++k) {
      const int j = lane + 64 * k;
      v[k] = j < J ? lt[p][j] : -INFINITY;
      m = fmaxf(m, v[k]);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < MAXD / 64; ++k) {
      v[k] = lane + 64 * k < J ? expf(v[k] - m) : 0.f;
      sum += v[k];
    }
    const float inv = 1.f / wave_sum(sum);
#pragma unroll
    for (int k = 0; k < MAXD / 64; ++k)
      if (lane + 64 * k < J) lt[p][lane + 64 * k] = v[k] * inv;
  }
  __syncthreads();
  const int p = t & 15;
  if (p0 + p < P)
    for (int j = t >> 4; j < J; j += 16) q[(int64_t)j * ld_q + col0 + p] = lt[p][j];
}

// ---- the products: C[b][m][n] = sum_k A[b][m][k] B[b][k][n] for any strides, 64 x 64 tile per workgroup (one 32 x 32 MFMA tile per
// wave), the contraction axis in steps of 16 through LDS; grid (ceil(N / 64), ceil(M / 64), B).  Elements outside M, N, K are never
// read (zero operands) or written.
constexpr int GT = 64, GK = 16, GLD = GT + 4;
enum { EPI_STORE = 0, EPI_ADD = 1, EPI_ROWBIAS = 2, EPI_SUBMUL = 3 };

struct GemmP {
  const float *A, *Bm, *D, *X, *bias;   // D: the addend (C's strides; may be C).  X: SUBMUL's factor.  bias [B][M]
  float* C;
  int64_t sAb, sAm, sAk, sBb, sBk, sBn, sCb, ldc, sXb, ldx;
  int M, N, K;
};

template <int EPI, bool SQ>
__global__ __launch_bounds__(256) void pgpool_gemm_kernel(const GemmP g) {
  __shared__ float As[GK][GLD], Bs[GK][GLD];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT, b = blockIdx.z;
  const float* A = g.A + (int64_t)b * g.sAb;
  const float* Bp = g.Bm + (int64_t)b * g.sBb;
  // a lane's four elements of each operand tile: the contraction index fastest where it is the contiguous one
  const bool akf = g.sAk == 1 && g.sAm != 1, bkf = g.sBk == 1 && g.sBn != 1;
  int ka[4], ra[4], kb[4], rb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ka[i] = akf ? (t & 15) : (t >> 6) + 4 * i;
    ra[i] = akf ? (t >> 4) + 16 * i : (t & 63);
    kb[i] = bkf ? (t & 15) : (t >> 6) + 4 * i;
    rb[i] = bkf ? (t >> 4) + 16 * i : (t & 63);
  }
  float va[4], vb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + ra[i], n = n0 + rb[i];
      float a = (m < g.M && k0 + ka[i] < g.K) ? A[(int64_t)m * g.sAm + (int64_t)(k0 + ka[i]) * g.sAk] : 0.f;
      if (SQ) a *= a;
      va[i] = a;
      vb[i] = (n < g.N && k0 + kb[i] < g.K) ? Bp[(int64_t)(k0 + kb[i]) * g.sBk + (int64_t)n * g.sBn] : 0.f;
    }
  };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  load(0);
  for (int k0 = 0; k0 < g.K; k0 += GK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      As[ka[i]][ra[i]] = va[i];
      Bs[kb[i]][rb[i]] = vb[i];
    }
    __syncthreads();
    if (k0 + GK < g.K) load(k0 + GK);
#pragma unroll
    for (int kk = 0; kk < GK / 2; ++kk) {
      const float a = As[2 * kk + (lane >> 5)][wm * 32 + (lane & 31)];
      const float bv = Bs[2 * kk + (lane >> 5)][wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
    }
    __syncthreads();                               // the tiles are rewritten by the next step
  }
  const int n = n0 + wn * 32 + (lane & 31);
  if (n >= g.N) return;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + wm * 32 + mfma_row(reg, lane >> 5);
    if (m >= g.M) continue;
    const int64_t o = (int64_t)b * g.sCb + (int64_t)m * g.ldc + n;
    float v = acc[reg];
    if (EPI == EPI_ADD) v += g.D[o];
    if (EPI == EPI_ROWBIAS) v += g.bias[(int64_t)b * g.M + m];
    if (EPI == EPI_SUBMUL) v = g.D[o] - g.X[(int64_t)b * g.sXb + (int64_t)m * g.ldx + n] * v;
    g.C[o] = v;
  }
}

template <int EPI, bool SQ>
void gemm_launch(const GemmP& g, int B, hipStream_t s) {
  hipLaunchKernelGGL((pgpool_gemm_kernel<EPI, SQ>), dim3((g.N + GT - 1) / GT, (g.M + GT - 1) / GT, B), dim3(256), 0, s, g);
}

// out[b][j] = sum_p w[j][(b, p)]: one wave per (j, b), lane-strided then the xor tree.  grid (J, B)
__global__ __launch_bounds__(64) void pgpool_rowsum_kernel(const float* __restrict__ wmat, int64_t ld_w, int P, int J, float* __restrict__ out) {
  const int j = blockIdx.x, b = blockIdx.y;
  const float* row = wmat + (int64_t)j * ld_w + (int64_t)b * P;
  float v = 0.f;
  for (int p = threadIdx.x; p < P; p += 64) v += row[p];
  v = wave_sum(v);
  if (threadIdx.x == 0) out[(int64_t)b * J + j] = v;
}

// zp over S, n2, zn: grid (C, B), 256 lanes over j (two each)
__global__ __launch_bounds__(256) void pgpool_normalize_kernel(float* __restrict__ S, const float* __restrict__ qs,
                                                               const float* __restrict__ centers, const float* __restrict__ tab, int C, int J,
                                                               float* __restrict__ zn, float* __restrict__ n2) {
  __shared__ float red[4];
  const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
  const float* stab = tab + 3 * (int64_t)C * J;
  const int64_t base = ((int64_t)b * C + c) * J;
  float zp[2], sq = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = t + 256 * u;
    zp[u] = 0.f;
    if (j < J) {
      const float qv = qs[(int64_t)b * J + j];
      zp[u] = (S[base + j] - centers[c * J + j] * qv) / (stab[c * J + j] * qv);
      sq = fmaf(zp[u], zp[u], sq);
    }
  }
  sq = block_sum(sq, red);
  const float n = sqrtf(fmaxf(sq, EPS));
  if (t == 0) n2[(int64_t)b * C + c] = sq;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = t + 256 * u;
    if (j < J) {
      S[base + j] = zp[u];
      zn[base + j] = zp[u] / n;
    }
  }
}

// dS = dzp / (s qs), dzp = (dzn - zn <dzn, zn>) / n (dzn / n where the norm's clamp held): grid (C, B), 256 lanes over j
__global__ __launch_bounds__(256) void pgpool_normalize_bwd_kernel(const float* __restrict__ dzn, const float* __restrict__ zn,
                                                                   const float* __restrict__ n2, const float* __restrict__ qs,
                                                                   const float* __restrict__ tab, int C, int J, float* __restrict__ dS) {
  __shared__ float red[4];
  const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
  const float* stab = tab + 3 * (int64_t)C * J;
  const int64_t base = ((int64_t)b * C + c) * J;
  float d[2], z[2], dot = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = t + 256 * u;
    d[u] = z[u] = 0.f;
    if (j < J) {
      d[u] = dzn[base + j];
      z[u] = zn[base + j];
      dot = fmaf(d[u], z[u], dot);
    }
  }
  dot = block_sum(dot, red);
  const float sq = n2[(int64_t)b * C + c], n = sqrtf(fmaxf(sq, EPS));
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = t + 256 * u;
    if (j < J) {
      const float dzp = (sq > EPS ? d[u] - z[u] * dot : d[u]) / n;
      dS[base + j] = dzp / (stab[c * J + j] * qs[(int64_t)b * J + j]);
    }
  }
}

// dqs[b][j] = -sum_c dS (S / qs), S / qs = zp s + centers: grid (ceil(J / 64), B), 64 lanes over j, the channels in order
__global__ __launch_bounds__(64) void pgpool_dqs_kernel(const float* __restrict__ dS, const float* __restrict__ zp, const float* __restrict__ centers,
                                                        const float* __restrict__ tab, int C, int J, float* __restrict__ dqs) {
  const int j = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (j >= J) return;
  const float* stab = tab + 3 * (int64_t)C * J;
  float v = 0.f;
  for (int c = 0; c < C; ++c) {
    const int64_t o = ((int64_t)b * C + c) * J + j;
    v = fmaf(dS[o], fmaf(zp[o], stab[c * J + j], centers[c * J + j]), v);
  }
  dqs[(int64_t)b * J + j] = -v;
}

// dl over dq: one column per lane.  grid (ceil(P / 256), B)
__global__ __launch_bounds__(256) void pgpool_softmax_bwd_kernel(const float* __restrict__ q, int64_t ld_q, const uint32_t* __restrict__ clamp,
                                                                 int W, float* __restrict__ dq, int64_t ld_dq, int P, int J) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  const int64_t col = (int64_t)b * P + p;
  float s = 0.f;
  for (int j = 0; j < J; ++j) s = fmaf(q[(int64_t)j * ld_q + col], dq[(int64_t)j * ld_dq + col], s);
  uint32_t bits = 0;
  for (int j = 0; j < J; ++j) {
    if ((j & 31) == 0) bits = clamp[col * W + (j >> 5)];
    const float v = q[(int64_t)j * ld_q + col] * (dq[(int64_t)j * ld_dq + col] - s);
    dq[(int64_t)j * ld_dq + col] = ((bits >> (j & 31)) & 1u) ? 0.f : v;
  }
}

// one (c, j) per lane, the samples in order (fp64)
__global__ __launch_bounds__(256) void pgpool_param_grad_kernel(const float* __restrict__ M0, const float* __restrict__ M1,
                                                                const float* __restrict__ M2, const float* __restrict__ dS,
                                                                const float* __restrict__ qs, const float* __restrict__ zp,
                                                                const float* __restrict__ centers, const float* __restrict__ tab, int B,
                                                                int C, int J, float* __restrict__ dcenters, float* __restrict__ dvariance) {
  const int n = C * J, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int j = e % J;
  const float r = tab[e], r2 = tab[n + e], s = tab[3 * n + e], cen = centers[e];
  double dc = 0.0, ds = 0.0;
  for (int b = 0; b < B; ++b) {
    const int64_t o = (int64_t)b * n + e;
    const float m0 = M0[(int64_t)b * J + j], m1 = M1[o], m2 = M2[o], pooled = dS[o] * qs[(int64_t)b * J + j];
    dc += (double)(r2 * (m1 - cen * m0) - pooled);
    ds += (double)(r2 * r * (m2 - 2.f * cen * m1 + cen * cen * m0) - pooled * zp[o]);
  }
  dcenters[e] = (float)dc;
  dvariance[e] = (float)ds * s * (1.f - s);
}

int dims_check(const char* what, int B, int64_t P, int C, int J) {
  SAR_REQUIRE(B >= 1 && P >= 1 && C >= 1 && J >= 1, "%s: need B, P, C, J >= 1 (got %d, %lld, %d, %d)", what, B, (long long)P, C, J);
  if (C > MAXD || J > MAXD) {
    sar_set_error("%s: built for C <= %d and J <= %d (got C = %d, J = %d)", what, MAXD, MAXD, C, J);
    return SAR_E_UNSUP;
  }
  if (B > 65535 || (int64_t)B * P >= ((int64_t)1 << 31) || (P + ATP - 1) / ATP >= ((int64_t)1 << 31)) {
    sar_set_error("%s: built for B <= 65535 and B * P < 2^31 (got B = %d, P = %lld)", what, B, (long long)P);
    return SAR_E_UNSUP;
  }
  return 0;
}

}  // namespace

#define PGPOOL_DIMS(name)                                 \
  if (int rc__ = dims_check(name, B, P, C, J)) return rc__

extern "C" int sar_pgpool_clamp_words(int J) { return J < 1 ? 0 : 2 * ((J + 63) / 64); }

extern "C" int sar_pgpool_prep_f32(const float* centers, const float* variance, int C, int J, float* tab, sar_stream_t s) {
  const int B = 1;
  const int64_t P = 1;
  PGPOOL_DIMS("sar_pgpool_prep_f32");
  SAR_REQUIRE(centers && variance && tab, "sar_pgpool_prep_f32: null operand");
  hipLaunchKernelGGL(pgpool_prep_kernel, dim3((C * J + 255) / 256), dim3(256), 0, as_stream(s), centers, variance, C * J, tab);
  SAR_LAUNCH_CHECK("sar_pgpool_prep_f32");
  return 0;
}

extern "C" int sar_pgpool_assign_f32(const float* x, int64_t ld_x, int B, int64_t P, int C, int J, const float* centers, const float* tab,
                                     float* q, int64_t ld_q, uint32_t* clamp, sar_stream_t s) {
  PGPOOL_DIMS("sar_pgpool_assign_f32");
  SAR_REQUIRE(x && centers && tab && q && clamp, "sar_pgpool_assign_f32: null operand");
  SAR_REQUIRE(ld_x >= (int64_t)B * P && ld_q >= (int64_t)B * P, "sar_pgpool_assign_f32: ld_x / ld_q below B * P");
  const dim3 grid((unsigned)((P + ATP - 1) / ATP), B);
  const int W = sar_pgpool_clamp_words(J);
  if (J > 256)
    hipLaunchKernelGGL(pgpool_assign_kernel<2>, grid, dim3(256), 0, as_stream(s), x, ld_x, (int)P, C, J, centers, tab, q, ld_q, clamp, W);
  else
    hipLaunchKernelGGL(pgpool_assign_kernel<1>, grid, dim3(256), 0, as_stream(s), x, ld_x, (int)P, C, J, centers, tab, q, ld_q, clamp, W);
  SAR_LAUNCH_CHECK("sar_pgpool_assign_f32");
  return 0;
}

extern "C" int sar_pgpool_moment_f32(const float* x, int64_t ld_x, const float* w, int64_t ld_w, int B, int64_t P, int C, int J, int square,
                                     float* out, sar_stream_t s) {
  PGPOOL_DIMS("sar_pgpool_moment_f32");
  SAR_REQUIRE(x && w && out, "sar_pgpool_moment_f32: null operand");
  SAR_REQUIRE(ld_x >= (int64_t)B * P && ld_w >= (int64_t)B * P, "sar_pgpool_moment_f32: ld_x / ld_w below B * P");
  GemmP g = {};
  g.A = x, g.sAb = P, g.sAm = ld_x, g.sAk = 1;
  g.Bm = w, g.sBb = P, g.sBk = 1, g.sBn = ld_w;
  g.C = out, g.sCb = (int64_t)C * J, g.ldc = J;
  g.M = C, g.N = J, g.K = (int)P;
  if (square)
    gemm_launch<EPI_STORE, true>(g, B, as_stream(s));
  else
    gemm_launch<EPI_STORE, false>(g, B, as_stream(s));
  SAR_LAUNCH_CHECK("sar_pgpool_moment_f32");
  return 0;
}

extern "C" int sar_pgpool_rowsum_f32(const float* w, int64_t ld_w, int B, int64_t P, int J, float* out, sar_stream_t s) {
  const int C = 1;
  PGPOOL_DIMS("sar_pgpool_rowsum_f32");
  SAR_REQUIRE(w && out, "sar_pgpool_rowsum_f32: null operand");
  SAR_REQUIRE(ld_w >= (int64_t)B * P, "sar_pgpool_rowsum_f32: ld_w below B * P");
  hipLaunchKernelGGL(pgpool_rowsum_kernel, dim3(J, B), dim3(64), 0, as_stream(s), w, ld_w, (int)P, J, out);
  SAR_LAUNCH_CHECK("sar_pgpool_rowsum_f32");
  return 0;
}

extern "C" int sar_pgpool_normalize_f32(float* S, const float* qs, const float* centers, const float* tab, int B, int C, int J, float* zn,
                                        float* n2, sar_stream_t s) {
  const int64_t P = 1;
  PGPOOL_DIMS("sar_pgpool_normalize_f32");
  SAR_REQUIRE(S && qs && centers && tab && zn && n2, "sar_pgpool_normalize_f32: null operand");
  hipLaunchKernelGGL(pgpool_normalize_kernel, dim3(C, B), dim3(256), 0, as_stream(s), S, qs, centers, tab, C, J, zn, n2);
  SAR_LAUNCH_CHECK("sar_pgpool_normalize_f32");
  return 0;
}

extern "C" int sar_pgpool_gram_f32(const float* zn, int B, int C, int J, float* A_out, sar_stream_t s) {
  const int64_t P = 1;
  PGPOOL_DIMS("sar_pgpool_gram_f32");
  SAR_REQUIRE(zn && A_out, "sar_pgpool_gram_f32: null operand");
  GemmP g = {};
  g.A = zn, g.sAb = (int64_t)C * J, g.sAm = 1, g.sAk = J;
  g.Bm = zn, g.sBb = (int64_t)C * J, g.sBk = J, g.sBn = 1;
  g.C = A_out, g.sCb = (int64_t)J * J, g.ldc = J;
  g.M = J, g.N = J, g.K = C;
  gemm_launch<EPI_STORE, false>(g, B, as_stream(s));
  SAR_LAUNCH_CHECK("sar_pgpool_gram_f32");
  return 0;
}

extern "C" int sar_pgpool_gram_bwd_f32(const float* zn, const float* dz, const float* dA, int B, int C, int J, float* dzn, sar_stream_t s) {
  const int64_t P = 1;
  PGPOOL_DIMS("sar_pgpool_gram_bwd_f32");
  SAR_REQUIRE(zn && dz && dA && dzn, "sar_pgpool_gram_bwd_f32: null operand");
  GemmP g = {};
  g.A = zn, g.sAb = (int64_t)C * J, g.sAm = J, g.sAk = 1;
  g.Bm = dA, g.sBb = (int64_t)J * J, g.sBk = J, g.sBn = 1;
  g.C = dzn, g.D = dz, g.sCb = (int64_t)C * J, g.ldc = J;
  g.M = C, g.N = J, g.K = J;
  gemm_launch<EPI_ADD, false>(g, B, as_stream(s));          // dz + zn dA
  g.sBk = 1, g.sBn = J, g.D = dzn;
  gemm_launch<EPI_ADD, false>(g, B, as_stream(s));          // + zn dA^T (each element read and written by one lane)
  SAR_LAUNCH_CHECK("sar_pgpool_gram_bwd_f32");
  return 0;
}

extern "C" int sar_pgpool_normalize_bwd_f32(const float* dzn, const float* zn, const float* zp, const float* n2, const float* qs,
                                            const float* centers, const float* tab, int B, int C, int J, float* dS, float* dqs,
                                            sar_stream_t s) {
  const int64_t P = 1;
  PGPOOL_DIMS("sar_pgpool_normalize_bwd_f32");
  SAR_REQUIRE(dzn && zn && zp && n2 && qs && centers && tab && dS && dqs, "sar_pgpool_normalize_bwd_f32: null operand");
  hipLaunchKernelGGL(pgpool_normalize_bwd_kernel, dim3(C, B), dim3(256), 0, as_stream(s), dzn, zn, n2, qs, tab, C, J, dS);
  hipLaunchKernelGGL(pgpool_dqs_kernel, dim3((J + 63) / 64, B), dim3(64), 0, as_stream(s), dS, zp, centers, tab, C, J, dqs);
  SAR_LAUNCH_CHECK("sar_pgpool_normalize_bwd_f32");
  return 0;
}

extern "C" int sar_pgpool_dq_f32(const float* x, int64_t ld_x, const float* dS, const float* dqs, int B, int64_t P, int C, int J, float* dq,
                                 int64_t ld_dq, sar_stream_t s) {
  PGPOOL_DIMS("sar_pgpool_dq_f32");
  SAR_REQUIRE(x && dS && dqs && dq, "sar_pgpool_dq_f32: null operand");
  SAR_REQUIRE(ld_x >= (int64_t)B * P && ld_dq >= (int64_t)B * P, "sar_pgpool_dq_f32: ld_x / ld_dq below B * P");
  GemmP g = {};
  g.A = dS, g.sAb = (int64_t)C * J, g.sAm = 1, g.sAk = J;
  g.Bm = x, g.sBb = P, g.sBk = ld_x, g.sBn = 1;
  g.C = dq, g.sCb = P, g.ldc = ld_dq, g.bias = dqs;
  g.M = J, g.N = (int)P, g.K = C;
  gemm_launch<EPI_ROWBIAS, false>(g, B, as_stream(s));
  SAR_LAUNCH_CHECK("sar_pgpool_dq_f32");
  return 0;
}

extern "C" int sar_pgpool_softmax_bwd_f32(const float* q, int64_t ld_q, const uint32_t* clamp, int B, int64_t P, int J, float* dq,
                                          int64_t ld_dq, sar_stream_t s) {
  const int C = 1;
  PGPOOL_DIMS("sar_pgpool_softmax_bwd_f32");
  SAR_REQUIRE(q && clamp && dq, "sar_pgpool_softmax_bwd_f32: null operand");
  SAR_REQUIRE(ld_q >= (int64_t)B * P && ld_dq >= (int64_t)B * P, "sar_pgpool_softmax_bwd_f32: ld_q / ld_dq below B * P");
  hipLaunchKernelGGL(pgpool_softmax_bwd_kernel, dim3((unsigned)((P + 255) / 256), B), dim3(256), 0, as_stream(s), q, ld_q, clamp,
                     sar_pgpool_clamp_words(J), dq, ld_dq, (int)P, J);
  SAR_LAUNCH_CHECK("sar_pgpool_softmax_bwd_f32");
  return 0;
}

extern "C" int sar_pgpool_dx_f32(const float* x, int64_t ld_x, const float* dS, const float* q, int64_t ld_q, const float* dl, int64_t ld_dl,
                                 const float* tab, int B, int64_t P, int C, int J, float* dx, int64_t ld_dx, sar_stream_t s) {
  PGPOOL_DIMS("sar_pgpool_dx_f32");
  SAR_REQUIRE(x && dS && q && dl && tab && dx && dx != x, "sar_pgpool_dx_f32: null operand, or dx is x");
  SAR_REQUIRE(ld_x >= (int64_t)B * P && ld_q >= (int64_t)B * P && ld_dl >= (int64_t)B * P && ld_dx >= (int64_t)B * P,
              "sar_pgpool_dx_f32: a leading dimension is below B * P");
  const int64_t n = (int64_t)C * J;
  GemmP g = {};
  g.A = dS, g.sAb = n, g.sAm = J, g.sAk = 1;
  g.Bm = q, g.sBb = P, g.sBk = ld_q, g.sBn = 1;
  g.C = dx, g.D = dx, g.sCb = P, g.ldc = ld_dx;
  g.X = x, g.sXb = P, g.ldx = ld_x;
  g.M = C, g.N = (int)P, g.K = J;
  gemm_launch<EPI_STORE, false>(g, B, as_stream(s));        // dS q
  g.A = tab + 2 * n, g.sAb = 0, g.Bm = dl, g.sBk = ld_dl;
  gemm_launch<EPI_ADD, false>(g, B, as_stream(s));          // + (r^2 centers) dl
  g.A = tab + n;
  gemm_launch<EPI_SUBMUL, false>(g, B, as_stream(s));       // - x * (r^2 dl)
  SAR_LAUNCH_CHECK("sar_pgpool_dx_f32");
  return 0;
}

extern "C" int sar_pgpool_param_grad_f32(const float* M0, const float* M1, const float* M2, const float* dS, const float* qs, const float* zp,
                                         const float* centers, const float* tab, int B, int C, int J, float* dcenters, float* dvariance,
                                         sar_stream_t s) {
  const int64_t P = 1;
  PGPOOL_DIMS("sar_pgpool_param_grad_f32");
  SAR_REQUIRE(M0 && M1 && M2 && dS && qs && zp && centers && tab && dcenters && dvariance, "sar_pgpool_param_grad_f32: null operand");
  hipLaunchKernelGGL(pgpool_param_grad_kernel, dim3((C * J + 255) / 256), dim3(256), 0, as_stream(s), M0, M1, M2, dS, qs, zp, centers, tab,
                     B, C, J, dcenters, dvariance);
  SAR_LAUNCH_CHECK("sar_pgpool_param_grad_f32");
  return 0;
}
