// gpool.hip -- GPool(keeprate), the top-k graph pooling of Graph U-Nets (models/stgcn_debug.py:29-72), fp32, forward and backward.
// x (N, C, T, V) and A (N, K, V, V); 1 <= V <= 64, 1 <= K <= 8, 1 <= keep <= V, N <= 65535, fewer than 2^31 elements per tensor.
//
//   ph   = p rsqrt(max(sum p^2, 1e-12))                             y[n, v] = sum_{c,t} x[n, c, t, v] ph[c T + t]
//   idx[n, :] = the keep vertices of largest y[n, :], descending, equal scores in ascending vertex index, NaN below every number
//   s[n, i] = sigmoid(y[n, idx_i])      out[n, c, t, i] = x[n, c, t, idx_i] s[n, i]      A_out[n, k] = (A[n, k]^2)[idx, idx]
//
// Addressing: element (n, c, t, v) of x / dx is at n s_n + c s_c + t V + v (of out / dout: t keep + i), so the modules' NCHW tensors
// (s_n = C T V, s_c = T V) and the engines' CN matrices [C][ld] (s_n = T V, s_c = ld) are served by the same kernels.  The run of
// T V floats of one (n, c) is contiguous, its start aligned to 4 bytes only (V = 25: 100-byte rows): every access is one dword of
// one lane under a predicate, there are no vector loads and no scalar tails.
//
// The kernels that walk x own one (sample, group of CC channels) per workgroup, CC = gp_group(T) a function of T alone.  Of the 256
// lanes L = (256 / W) W are live (W = V, or keep where the rows are the pooled ones): lane -> (tt, w) = (lane / W, lane % W), fixed for
// the whole walk, and one step of the walk is 256 / W consecutive rows = L consecutive floats.  No index is divided inside a loop.
//
//   prep      ph, sum p^2 and 1 / max(|p|, 1e-6) (one workgroup, fp64)
//   score     part[n][g][v] = the group's share of y: per lane one fmaf chain over its rows (fp32), the 256 / V lanes of a vertex
//             added in lane order in fp64.  Every vertex's sum is the same sequence of operations on its own column: two bitwise
//             equal joints get bitwise equal scores
//   select    one wave per sample, one lane per vertex: y = the groups in order (fp64), rank by counting
//             rank(v) = #{u : y_u > y_v or (y_u == y_v and u < v)} with NaN last -- a total order, so idx[n] is keep distinct
//             vertices whatever the scores are; idx, s, y and pos (pos[n][v] = i where v = idx[n][i], else -1)
//   gather    out
//   adj       A_out[n, k][i][j] = sum_u A[idx_i][u] A[u][idx_j], one fmaf chain over u per element, A[n, k] in LDS
//   ds        dspart[n][g][i] = the group's share of sum_{c,t} dout[n, c, t, i] x[n, c, t, idx_i] (as score)
//   dy        dy[n][idx_i] = ds s (1 - s) (ds = the groups in order, fp64), 0 elsewhere
//   dx        dx[n, c, t, v] = (v = idx_i ? dout[n, c, t, i] s[n, i] : 0) + dy[n, v] ph[c T + t]: every element written; and
//             dphp[n][c T + t] = sum_{v selected} dy[n, v] x[n, c, t, v] (the row's products through LDS, added in vertex order)
//   dp        dph[ct] = sum_n dphp[n][ct] in sample order (fp64); dp = (dph - ph <dph, ph>) / |p| (dph 1e6 where sum p^2 <= 1e-12)
//   adj_bwd   dA[n, k] = G A^T + A^T G, G = dA_out scattered to (idx_i, idx_j): two fmaf chains per element
// No atomics; every sum has one fixed order; everything but dp is computed from the sample's own data by workgroups whose work does
// not depend on N: bitwise deterministic, and a sample's results do not depend on the rest of the batch.
#include "sar_common.h"

namespace {

constexpr int TPB = 256;
constexpr int GP_ROWS = 1024;                 // rows (c, t) per workgroup, about
constexpr int GP_U = 8;                       // steps of the dx walk between two row sums
constexpr int GP_AS = SAR_GPOOL_VMAX + 1;     // LDS row stride of an adjacency

inline int gp_group(int T) { return T >= GP_ROWS ? 1 : (GP_ROWS + T - 1) / T; }
inline int gp_ngroups(int C, int T) { return (C + gp_group(T) - 1) / gp_group(T); }

// a strided (N, C, T, W) tensor: the run of (n, c) starts at p + n sn + c sc
struct gp_view {
  const float* p;
  int64_t sn, sc;
};
struct gp_wview {
  float* p;
  int64_t sn, sc;
};

__global__ __launch_bounds__(TPB) void gp_prep_kernel(const float* __restrict__ p, int CT, float* __restrict__ ph, float* __restrict__ norm) {
  __shared__ double red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < CT; i += TPB) a += (double)p[i] * (double)p[i];
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  const double n2 = (red[0] + red[1]) + (red[2] + red[3]);
  const float inv = (float)(1.0 / sqrt(fmax(n2, 1e-12)));
  for (int i = threadIdx.x; i < CT; i += TPB) ph[i] = p[i] * inv;
  if (threadIdx.x == 0) norm[0] = (float)n2, norm[1] = inv;
}

// grid (groups, N)
__global__ __launch_bounds__(TPB) void gp_score_kernel(const gp_view x, const float* __restrict__ ph, int C, int T, int V, int CC,
                                                       float* __restrict__ part) {
  __shared__ float red[TPB];
  const int G = TPB / V, tt = threadIdx.x / V, v = threadIdx.x - tt * V, n = blockIdx.y;
  const int c0 = blockIdx.x * CC, c1 = c0 + CC < C ? c0 + CC : C;
  float acc = 0.f;
  if (tt < G)
    for (int c = c0; c < c1; ++c) {
      const float* xr = x.p + n * x.sn + c * x.sc + v;
      const float* pr = ph + c * T;
#pragma unroll 4
      for (int t = tt; t < T; t += G) acc = fmaf(xr[t * V], pr[t], acc);
    }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < V) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)red[g * V + threadIdx.x];
    part[((int64_t)n * gridDim.x + blockIdx.x) * V + threadIdx.x] = (float)s;
  }
}

// a > b with NaN below every number
__device__ __forceinline__ bool gp_above(float a, float b) { return a == a && (b != b || a > b); }
__device__ __forceinline__ bool gp_same(float a, float b) { return a == b || (a != a && b != b); }

// grid N, one wave
__global__ __launch_bounds__(64) void gp_select_kernel(const float* __restrict__ part, int ng, int V, int keep, float* __restrict__ y,
                                                       int32_t* __restrict__ idx, float* __restrict__ sv, int32_t* __restrict__ pos) {
  __shared__ float ys[64];
  const int v = threadIdx.x, n = blockIdx.x;
  float yv = 0.f;
  if (v < V) {
    double s = 0.0;
    for (int g = 0; g < ng; ++g) s += (double)part[((int64_t)n * ng + g) * V + v];
    yv = (float)s;
    ys[v] = yv;
  }
  __syncthreads();
  if (v >= V) return;
  int rank = 0;
  for (int u = 0; u < V; ++u) {
    const float yu = ys[u];
    rank += (gp_above(yu, yv) || (gp_same(yu, yv) && u < v)) ? 1 : 0;
  }
  y[(int64_t)n * V + v] = yv;
  pos[(int64_t)n * V + v] = rank < keep ? rank : -1;
  if (rank < keep) {
    idx[(int64_t)n * keep + rank] = v;
    sv[(int64_t)n * keep + rank] = 1.f / (1.f + expf(-yv));
  }
}

// grid (groups, N); lane -> (tt, i)
__global__ __launch_bounds__(TPB) void gp_gather_kernel(const gp_view x, const int32_t* __restrict__ idx, const float* __restrict__ sv, int C,
                                                        int T, int V, int keep, int CC, const gp_wview out) {
  const int G = TPB / keep, tt = threadIdx.x / keep, i = threadIdx.x - tt * keep, n = blockIdx.y;
  if (tt >= G) return;
  const int c0 = blockIdx.x * CC, c1 = c0 + CC < C ? c0 + CC : C;
  const int vi = idx[(int64_t)n * keep + i];
  const float s = sv[(int64_t)n * keep + i];
  for (int c = c0; c < c1; ++c) {
    const float* xr = x.p + n * x.sn + c * x.sc + vi;
    float* o = out.p + n * out.sn + c * out.sc + i;
#pragma unroll 4
    for (int t = tt; t < T; t += G) o[t * keep] = xr[t * V] * s;
  }
}

// grid (groups, N); lane -> (tt, i)
__global__ __launch_bounds__(TPB) void gp_ds_kernel(const gp_view x, const gp_view dout, const int32_t* __restrict__ idx, int C, int T, int V,
                                                    int keep, int CC, float* __restrict__ part) {
  __shared__ float red[TPB];
  const int G = TPB / keep, tt = threadIdx.x / keep, i = threadIdx.x - tt * keep, n = blockIdx.y;
  const int c0 = blockIdx.x * CC, c1 = c0 + CC < C ? c0 + CC : C;
  float acc = 0.f;
  if (tt < G) {
    const int vi = idx[(int64_t)n * keep + i];
    for (int c = c0; c < c1; ++c) {
      const float* xr = x.p + n * x.sn + c * x.sc + vi;
      const float* dr = dout.p + n * dout.sn + c * dout.sc + i;
#pragma unroll 4
      for (int t = tt; t < T; t += G) acc = fmaf(dr[t * keep], xr[t * V], acc);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < keep) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)red[g * keep + threadIdx.x];
    part[((int64_t)n * gridDim.x + blockIdx.x) * keep + threadIdx.x] = (float)s;
  }
}

// grid N, one wave
__global__ __launch_bounds__(64) void gp_dy_kernel(const float* __restrict__ part, int ng, const float* __restrict__ sv,
                                                   const int32_t* __restrict__ idx, int V, int keep, float* __restrict__ dy) {
  __shared__ float ds[64];
  const int l = threadIdx.x, n = blockIdx.x;
  ds[l] = 0.f;
  __syncthreads();
  if (l < keep) {
    double a = 0.0;
    for (int g = 0; g < ng; ++g) a += (double)part[((int64_t)n * ng + g) * keep + l];
    const float s = sv[(int64_t)n * keep + l];
    ds[idx[(int64_t)n * keep + l]] = (float)a * s * (1.f - s);
  }
  __syncthreads();
  if (l < V) dy[(int64_t)n * V + l] = ds[l];
}

// grid (groups, N); lane -> (tt, v).  GP_U steps of the walk leave their products in LDS as rows [t][v]; then one lane per row adds
// the row in vertex order
__global__ __launch_bounds__(TPB) void gp_dx_kernel(const gp_view x, const gp_view dout, const int32_t* __restrict__ pos,
                                                    const float* __restrict__ sv, const float* __restrict__ dy, const float* __restrict__ ph,
                                                    int C, int T, int V, int keep, int CC, const gp_wview dx, float* __restrict__ dphp) {
  __shared__ float prod[GP_U * (TPB + TPB / 2)];       // GP_U G rows of stride V | 1 <= V + 1: G (V + 1) <= 256 + G, G <= 128 where V > 1
  const int G = TPB / V, tt = threadIdx.x / V, v = threadIdx.x - tt * V, n = blockIdx.y;
  const int VS = V | 1;
  const int c0 = blockIdx.x * CC, c1 = c0 + CC < C ? c0 + CC : C;
  const bool live = tt < G;
  int pi = -1;
  float s = 0.f, dyv = 0.f;
  if (live) {
    pi = pos[(int64_t)n * V + v];
    dyv = dy[(int64_t)n * V + v];
    if (pi >= 0) s = sv[(int64_t)n * keep + pi];
  }
  const int pj = pi >= 0 ? pi : 0;
  for (int c = c0; c < c1; ++c) {
    const float* xr = x.p + n * x.sn + c * x.sc + v;
    const float* dr = dout.p + n * dout.sn + c * dout.sc + pj;
    float* o = dx.p + n * dx.sn + c * dx.sc + v;
    const float* pr = ph + c * T;
    for (int tb = 0; tb < T; tb += GP_U * G) {
      __syncthreads();                                 // the previous rows have been added
      if (live) {
#pragma unroll
        for (int it = 0; it < GP_U; ++it) {
          const int r = it * G + tt, t = tb + r;
          if (t < T) {
            const float g = pi >= 0 ? dr[t * keep] * s : 0.f;
            o[t * V] = fmaf(dyv, pr[t], g);
            prod[r * VS + v] = pi >= 0 ? dyv * xr[t * V] : 0.f;
          }
        }
      }
      __syncthreads();
      for (int r = threadIdx.x; r < GP_U * G && tb + r < T; r += TPB) {
        float a = 0.f;
        for (int j = 0; j < V; ++j) a += prod[r * VS + j];
        dphp[(int64_t)n * C * T + (int64_t)c * T + tb + r] = a;
      }
    }
  }
}

// dph[ct] = the samples in order, fp64
__global__ __launch_bounds__(64) void gp_dph_kernel(const float* __restrict__ dphp, int N, int CT, float* __restrict__ dph) {
  const int ct = blockIdx.x * 64 + threadIdx.x;
  if (ct >= CT) return;
  double a = 0.0;
#pragma unroll 8
  for (int n = 0; n < N; ++n) a += (double)dphp[(int64_t)n * CT + ct];
  dph[ct] = (float)a;
}

// one workgroup: <dph, ph> in fp64, then dp
__global__ __launch_bounds__(TPB) void gp_dp_kernel(const float* __restrict__ dph, const float* __restrict__ ph, const float* __restrict__ norm,
                                                    int CT, float* __restrict__ dp) {
  __shared__ double red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < CT; i += TPB) a += (double)dph[i] * (double)ph[i];
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  const float dot = (float)((red[0] + red[1]) + (red[2] + red[3]));
  const float inv = norm[1];
  const bool clamped = !(norm[0] > 1e-12f);
  for (int i = threadIdx.x; i < CT; i += TPB) dp[i] = clamped ? dph[i] * inv : (dph[i] - ph[i] * dot) * inv;
}

// grid (K, N): A[n, k] in LDS
__global__ __launch_bounds__(TPB) void gp_adj_kernel(const float* __restrict__ A, const int32_t* __restrict__ idx, int V, int keep,
                                                     float* __restrict__ A_out) {
  __shared__ float As[SAR_GPOOL_VMAX * GP_AS];
  __shared__ int ids[SAR_GPOOL_VMAX];
  const int k = blockIdx.x, n = blockIdx.y, K = gridDim.x;
  const float* a = A + ((int64_t)n * K + k) * V * V;
  for (int e = threadIdx.x; e < V * V; e += TPB) As[(e / V) * GP_AS + e % V] = a[e];
  if (threadIdx.x < keep) ids[threadIdx.x] = idx[(int64_t)n * keep + threadIdx.x];
  __syncthreads();
  float* o = A_out + ((int64_t)n * K + k) * keep * keep;
  for (int e = threadIdx.x; e < keep * keep; e += TPB) {
    const int vi = ids[e / keep], vj = ids[e % keep];
    float acc = 0.f;
    for (int u = 0; u < V; ++u) acc = fmaf(As[vi * GP_AS + u], As[u * GP_AS + vj], acc);
    o[e] = acc;
  }
}

// grid (K, N): dA[a][b] = (a = idx_i ? sum_j G[i][j] A[b][idx_j] : 0) + (b = idx_j ? sum_i A[idx_i][a] G[i][j] : 0)
__global__ __launch_bounds__(TPB) void gp_adj_bwd_kernel(const float* __restrict__ A, const float* __restrict__ dA_out,
                                                         const int32_t* __restrict__ idx, const int32_t* __restrict__ pos, int V, int keep,
                                                         float* __restrict__ dA) {
  __shared__ float As[SAR_GPOOL_VMAX * GP_AS];
  __shared__ float Gs[SAR_GPOOL_VMAX * GP_AS];
  __shared__ int ids[SAR_GPOOL_VMAX], ps[SAR_GPOOL_VMAX];
  const int k = blockIdx.x, n = blockIdx.y, K = gridDim.x;
  const float* a = A + ((int64_t)n * K + k) * V * V;
  const float* g = dA_out + ((int64_t)n * K + k) * keep * keep;
  for (int e = threadIdx.x; e < V * V; e += TPB) As[(e / V) * GP_AS + e % V] = a[e];
  for (int e = threadIdx.x; e < keep * keep; e += TPB) Gs[(e / keep) * GP_AS + e % keep] = g[e];
  if (threadIdx.x < keep) ids[threadIdx.x] = idx[(int64_t)n * keep + threadIdx.x];
  if (threadIdx.x < V) ps[threadIdx.x] = pos[(int64_t)n * V + threadIdx.x];
  __syncthreads();
  float* o = dA + ((int64_t)n * K + k) * V * V;
  for (int e = threadIdx.x; e < V * V; e += TPB) {
    const int ra = e / V, cb = e % V, pa = ps[ra], pb = ps[cb];
    float left = 0.f, right = 0.f;
    if (pa >= 0)
      for (int j = 0; j < keep; ++j) left = fmaf(Gs[pa * GP_AS + j], As[cb * GP_AS + ids[j]], left);
    if (pb >= 0)
      for (int i = 0; i < keep; ++i) right = fmaf(As[ids[i] * GP_AS + ra], Gs[i * GP_AS + pb], right);
    o[e] = left + right;
  }
}

// every limit, before any launch
int gp_dims(const char* who, int N, int C, int T, int V, int keep) {
  SAR_REQUIRE(N >= 1 && C >= 1 && T >= 1 && V >= 1 && keep >= 1 && keep <= V, "%s: need N, C, T, V >= 1 and 1 <= keep <= V (got %d, %d, %d, %d, keep %d)",
              who, N, C, T, V, keep);
  if (V > SAR_GPOOL_VMAX || N > 65535 || (int64_t)N * C * T * V >= ((int64_t)1 << 31)) {
    sar_set_error("%s: built for V <= %d, N <= 65535 and N * C * T * V < 2^31 (got N = %d, C = %d, T = %d, V = %d)", who, SAR_GPOOL_VMAX, N, C,
                  T, V);
    return SAR_E_UNSUP;
  }
  return 0;
}

int gp_adj_dims(const char* who, int N, int K, int V, int keep) {
  SAR_REQUIRE(N >= 1 && K >= 1 && V >= 1 && keep >= 1 && keep <= V, "%s: need N, K, V >= 1 and 1 <= keep <= V (got %d, %d, %d, keep %d)", who, N,
              K, V, keep);
  if (V > SAR_GPOOL_VMAX || K > SAR_GPOOL_KMAX || N > 65535) {
    sar_set_error("%s: built for V <= %d, K <= %d and N <= 65535 (got N = %d, K = %d, V = %d)", who, SAR_GPOOL_VMAX, SAR_GPOOL_KMAX, N, K, V);
    return SAR_E_UNSUP;
  }
  return 0;
}

// the runs of W = T w floats of a strided (N, C, T, w) tensor lie inside it and do not overlap: channel-major inside the sample
// (NCHW) or sample-major inside the channel (CN)
bool gp_strides_ok(int64_t sn, int64_t sc, int N, int C, int64_t W) {
  const int64_t lim = (int64_t)1 << 31;
  if (sn < 1 || sc < 1 || sn >= lim || sc >= lim) return false;
  const bool nchw = sc >= W && (C == 1 || N == 1 || sn >= (int64_t)C * sc), cn = sn >= W && (N == 1 || C == 1 || sc >= (int64_t)N * sn);
  return (nchw || cn) && (N - 1) * sn + (C - 1) * sc + W <= lim;
}

}  // namespace

#define GP_DIMS(name)                                      \
  if (int rc__ = gp_dims(name, N, C, T, V, keep)) return rc__
#define GP_STRIDES(name, sn, sc, w)                                                                                  \
  SAR_REQUIRE(gp_strides_ok(sn, sc, N, C, (int64_t)T * (w)), "%s: strides (%lld, %lld) do not describe a (N, C, T, %d) tensor", name, \
              (long long)(sn), (long long)(sc), (int)(w))

extern "C" int sar_gpool_groups(int C, int T) { return (C < 1 || T < 1) ? SAR_E_ARG : gp_ngroups(C, T); }

extern "C" int sar_gpool_prep_f32(const float* p, int CT, float* ph, float* norm, sar_stream_t s) {
  SAR_REQUIRE(p && ph && norm && CT >= 1, "sar_gpool_prep_f32: null operand or CT < 1");
  hipLaunchKernelGGL(gp_prep_kernel, dim3(1), dim3(TPB), 0, as_stream(s), p, CT, ph, norm);
  SAR_LAUNCH_CHECK("sar_gpool_prep_f32");
  return 0;
}

extern "C" int sar_gpool_score_f32(const float* x, int64_t s_n, int64_t s_c, const float* ph, int N, int C, int T, int V, float* part,
                                   sar_stream_t s) {
  const int keep = 1;
  GP_DIMS("sar_gpool_score_f32");
  SAR_REQUIRE(x && ph && part, "sar_gpool_score_f32: null operand");
  GP_STRIDES("sar_gpool_score_f32", s_n, s_c, V);
  hipLaunchKernelGGL(gp_score_kernel, dim3(gp_ngroups(C, T), N), dim3(TPB), 0, as_stream(s), gp_view{x, s_n, s_c}, ph, C, T, V, gp_group(T),
                     part);
  SAR_LAUNCH_CHECK("sar_gpool_score_f32");
  return 0;
}

extern "C" int sar_gpool_select_f32(const float* part, int N, int C, int T, int V, int keep, float* y, int32_t* idx, float* sv, int32_t* pos,
                                    sar_stream_t s) {
  GP_DIMS("sar_gpool_select_f32");
  SAR_REQUIRE(part && y && idx && sv && pos, "sar_gpool_select_f32: null operand");
  hipLaunchKernelGGL(gp_select_kernel, dim3(N), dim3(64), 0, as_stream(s), part, gp_ngroups(C, T), V, keep, y, idx, sv, pos);
  SAR_LAUNCH_CHECK("sar_gpool_select_f32");
  return 0;
}

extern "C" int sar_gpool_gather_f32(const float* x, int64_t s_n, int64_t s_c, const int32_t* idx, const float* sv, int N, int C, int T, int V,
                                    int keep, float* out, int64_t o_sn, int64_t o_sc, sar_stream_t s) {
  GP_DIMS("sar_gpool_gather_f32");
  SAR_REQUIRE(x && idx && sv && out, "sar_gpool_gather_f32: null operand");
  GP_STRIDES("sar_gpool_gather_f32", s_n, s_c, V);
  GP_STRIDES("sar_gpool_gather_f32", o_sn, o_sc, keep);
  hipLaunchKernelGGL(gp_gather_kernel, dim3(gp_ngroups(C, T), N), dim3(TPB), 0, as_stream(s), gp_view{x, s_n, s_c}, idx, sv, C, T, V, keep,
                     gp_group(T), gp_wview{out, o_sn, o_sc});
  SAR_LAUNCH_CHECK("sar_gpool_gather_f32");
  return 0;
}

extern "C" int sar_gpool_adj_f32(const float* A, const int32_t* idx, int N, int K, int V, int keep, float* A_out, sar_stream_t s) {
  if (int rc = gp_adj_dims("sar_gpool_adj_f32", N, K, V, keep)) return rc;
  SAR_REQUIRE(A && idx && A_out, "sar_gpool_adj_f32: null operand");
  hipLaunchKernelGGL(gp_adj_kernel, dim3(K, N), dim3(TPB), 0, as_stream(s), A, idx, V, keep, A_out);
  SAR_LAUNCH_CHECK("sar_gpool_adj_f32");
  return 0;
}

extern "C" int sar_gpool_adj_bwd_f32(const float* A, const float* dA_out, const int32_t* idx, const int32_t* pos, int N, int K, int V,
                                     int keep, float* dA, sar_stream_t s) {
  if (int rc = gp_adj_dims("sar_gpool_adj_bwd_f32", N, K, V, keep)) return rc;
  SAR_REQUIRE(A && dA_out && idx && pos && dA, "sar_gpool_adj_bwd_f32: null operand");
  hipLaunchKernelGGL(gp_adj_bwd_kernel, dim3(K, N), dim3(TPB), 0, as_stream(s), A, dA_out, idx, pos, V, keep, dA);
  SAR_LAUNCH_CHECK("sar_gpool_adj_bwd_f32");
  return 0;
}

extern "C" int sar_gpool_ds_f32(const float* x, int64_t s_n, int64_t s_c, const float* dout, int64_t d_sn, int64_t d_sc, const int32_t* idx,
                                int N, int C, int T, int V, int keep, float* part, sar_stream_t s) {
  GP_DIMS("sar_gpool_ds_f32");
  SAR_REQUIRE(x && dout && idx && part, "sar_gpool_ds_f32: null operand");
  GP_STRIDES("sar_gpool_ds_f32", s_n, s_c, V);
  GP_STRIDES("sar_gpool_ds_f32", d_sn, d_sc, keep);
  hipLaunchKernelGGL(gp_ds_kernel, dim3(gp_ngroups(C, T), N), dim3(TPB), 0, as_stream(s), gp_view{x, s_n, s_c}, gp_view{dout, d_sn, d_sc}, idx,
                     C, T, V, keep, gp_group(T), part);
  SAR_LAUNCH_CHECK("sar_gpool_ds_f32");
  return 0;
}

extern "C" int sar_gpool_dy_f32(const float* part, const float* sv, const int32_t* idx, int N, int C, int T, int V, int keep, float* dy,
                                sar_stream_t s) {
  GP_DIMS("sar_gpool_dy_f32");
  SAR_REQUIRE(part && sv && idx && dy, "sar_gpool_dy_f32: null operand");
  hipLaunchKernelGGL(gp_dy_kernel, dim3(N), dim3(64), 0, as_stream(s), part, gp_ngroups(C, T), sv, idx, V, keep, dy);
  SAR_LAUNCH_CHECK("sar_gpool_dy_f32");
  return 0;
}

extern "C" int sar_gpool_dx_f32(const float* x, int64_t s_n, int64_t s_c, const float* dout, int64_t d_sn, int64_t d_sc, const int32_t* pos,
                                const float* sv, const float* dy, const float* ph, int N, int C, int T, int V, int keep, float* dx,
                                int64_t g_sn, int64_t g_sc, float* dphp, sar_stream_t s) {
  GP_DIMS("sar_gpool_dx_f32");
  SAR_REQUIRE(x && dout && pos && sv && dy && ph && dx && dphp && dx != x, "sar_gpool_dx_f32: null operand, or dx is x");
  GP_STRIDES("sar_gpool_dx_f32", s_n, s_c, V);
  GP_STRIDES("sar_gpool_dx_f32", d_sn, d_sc, keep);
  GP_STRIDES("sar_gpool_dx_f32", g_sn, g_sc, V);
  hipLaunchKernelGGL(gp_dx_kernel, dim3(gp_ngroups(C, T), N), dim3(TPB), 0, as_stream(s), gp_view{x, s_n, s_c}, gp_view{dout, d_sn, d_sc}, pos,
                     sv, dy, ph, C, T, V, keep, gp_group(T), gp_wview{dx, g_sn, g_sc}, dphp);
  SAR_LAUNCH_CHECK("sar_gpool_dx_f32");
  return 0;
}

extern "C" int sar_gpool_dp_f32(const float* dphp, const float* ph, const float* norm, int N, int CT, float* dph, float* dp, sar_stream_t s) {
  SAR_REQUIRE(dphp && ph && norm && dph && dp && N >= 1 && CT >= 1, "sar_gpool_dp_f32: null operand, or N or CT < 1");
  if (N > 65535 || (int64_t)N * CT >= ((int64_t)1 << 31)) {
    sar_set_error("sar_gpool_dp_f32: built for N <= 65535 and N * CT < 2^31 (got N = %d, CT = %d)", N, CT);
    return SAR_E_UNSUP;
  }
  hipLaunchKernelGGL(gp_dph_kernel, dim3((CT + 63) / 64), dim3(64), 0, as_stream(s), dphp, N, CT, dph);
  hipLaunchKernelGGL(gp_dp_kernel, dim3(1), dim3(TPB), 0, as_stream(s), dph, ph, norm, CT, dp);
  SAR_LAUNCH_CHECK("sar_gpool_dp_f32");
  return 0;
}
