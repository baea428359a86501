// adjattn.hip -- the adaptive adjacency of 2s-AGCN (the C_k term), fp32, forward and backward.
// theta, phi: CN matrices [K Ce][ld] with columns (n, t, v), ld >= N T V; channel k Ce + e belongs to subset k.
//
//   S[n,k,v,w]     = (1 / (Ce T)) sum_{e,t} theta[k Ce + e][n,t,v] phi[k Ce + e][n,t,w]
//   P[n,k,:,w]     = softmax over v of S[n,k,:,w]                A_eff[n,k,v,w] = A[k,v,w] + P[n,k,v,w]
//   g[n,k,w]       = sum_v P dA_eff      dS = P (dA_eff - g)     dA[k] = sum_n dA_eff[n,k]
//   dtheta[k Ce + e][n,t,v] = (1 / (Ce T)) sum_w dS[n,k,v,w] phi[k Ce + e][n,t,w]
//   dphi  [k Ce + e][n,t,w] = (1 / (Ce T)) sum_v dS[n,k,v,w] theta[k Ce + e][n,t,v]
//
// The run of T V floats of one embedding channel of one sample is contiguous, so every operand of the two products goes from global
// memory (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation) without a transposed copy: the similarity straight into the
// operand registers, the embeddings' gradient through an LDS image of the rows as they lie.
//
//   sim      grid (N K, slabs).  One MFMA step is two frames of one embedding channel: lane l takes theta[e][(t0 + (l >> 5)) V + (l & 31)]
//            as its A element and the same address of phi as its B element, each under (l & 31) < V and t0 + (l >> 5) < T, so the
//            32 x 32 accumulator is the V x V block of S.  The Ce ceil(T / 2) steps of a (n, k) are cut into sar_adjattn_sim_slabs(Ce, T, V)
//            runs, a run into four for the waves of a workgroup -- a function of (Ce, T) alone.  The four wave partials are added in
//            wave order in fp64; with one slab that sum is divided by Ce T and is S, with more it is the slab's partial and a second
//            launch adds the slabs in slab order in fp64 and divides.
//   softmax / softmax_bwd   one lane per column (n, k, w), walking v; the column maximum is subtracted, expf; g is summed in fp64.
//            dA[k] is one lane per element, summing the samples in order in fp64.
//   dembed   grid (N K, chunks).  A tile is 32 frames of one embedding channel.  dS[n,k] and its transpose stay in 2 x 16 VGPRs as the
//            B operands of all 16 steps of every tile of the workgroup; wave w owns tiles 4 chunk + w, + 4 chunks, ...  The tile's
//            contiguous run of 32 V floats of theta and of phi goes global -> registers (coalesced, under the previous tile's MFMAs)
//            -> the wave's own LDS image, from which a lane reads its row's operand of each step (row stride V: conflict-free for
//            an odd V); dtheta and dphi are written once from the accumulators with the 1 / (Ce T) factor.
// No atomics; every sum has one fixed order that depends on (Ce, T, V) only: bitwise deterministic, and a sample's S / P / dS / dtheta /
// dphi do not depend on the rest of the batch.
#include "sar_common.h"

namespace {

constexpr int TPB = 256;
constexpr int AA_VMAX = SAR_ADJATTN_VMAX, AA_KMAX = SAR_ADJATTN_KMAX, AA_EMAX = SAR_ADJATTN_EMAX;
constexpr int SIM_U = 8;             // steps of the similarity whose operands are in flight at once
constexpr int SIM_SLAB_STEPS = 512;  // a slab is about this many steps ..
constexpr int SIM_SLAB_MAX = 8;      // .. and there are at most this many slabs
constexpr int DE_TR = 32;            // frames of a dembed tile
constexpr int DE_TILES = 16;         // tiles a dembed workgroup aims at (4 per wave)
constexpr int DE_CHUNK_MAX = 1024;

// grid (N K, slabs): steps [blockIdx.y sps, ..) of the nsteps = Ce npairs steps of (n, k); step s = (channel s / npairs, frames 2 (s % npairs) ..)
__global__ __launch_bounds__(TPB) void aa_sim_kernel(const float* __restrict__ theta, const float* __restrict__ phi, int64_t ld, int K, int Ce,
                                                     int T, int V, int npairs, int sps, int nsteps, double denom, float* __restrict__ out,
                                                     int64_t slab_stride) {
  __shared__ float red[4][32 * 32];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lo = lane & 31, hi = lane >> 5;
  const int nk = blockIdx.x, n = nk / K, k = nk - n * K;
  const int b0 = blockIdx.y * sps, b1 = b0 + sps < nsteps ? b0 + sps : nsteps;
  const int q = (b1 - b0 + 3) >> 2;
  int s = b0 + w * q;
  const int s1 = s + q < b1 ? s + q : b1;
  f32x16 acc;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
  if (s < s1) {
    const bool lv = lo < V;
    const int e0 = s / npairs;
    int pr = s - e0 * npairs;
    const int64_t at = ((int64_t)k * Ce + e0) * ld + (int64_t)n * T * V + lo;
    const float* th = theta + at;
    const float* ph = phi + at;
    for (; s < s1; s += SIM_U) {
      float a[SIM_U], b[SIM_U];
#pragma unroll
      for (int u = 0; u < SIM_U; ++u) {
        const bool live = s + u < s1;            // (wave-uniform)
        const int t = 2 * pr + hi;
        const bool ok = live && lv && t < T;
        a[u] = ok ? th[t * V] : 0.f;
        b[u] = ok ? ph[t * V] : 0.f;
        if (live && ++pr == npairs) pr = 0, th += ld, ph += ld;
      }
#pragma unroll
      for (int u = 0; u < SIM_U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) red[w][mfma_row(reg, hi) * 32 + lo] = acc[reg];
  __syncthreads();
  float* o = out + blockIdx.y * slab_stride + (int64_t)nk * V * V;
  for (int idx = tid; idx < 32 * 32; idx += TPB) {
    const int v = idx >> 5, ww = idx & 31;
    if (v < V && ww < V) {
      double sum = (double)red[0][idx];
      sum += (double)red[1][idx];
      sum += (double)red[2][idx];
      sum += (double)red[3][idx];
      o[v * V + ww] = (float)(sum / denom);
    }
  }
}

// grid ceil(n / 256): S[i] = (sum of the slabs in slab order, fp64) / denom
__global__ __launch_bounds__(TPB) void aa_sim_finish_kernel(const float* __restrict__ slab, int nslab, int64_t stride, int64_t n, double denom,
                                                            float* __restrict__ S) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  double sum = 0.0;
  for (int j = 0; j < nslab; ++j) sum += (double)slab[j * stride + i];
  S[i] = (float)(sum / denom);
}

// grid ceil(N K V / 256): one lane per column (n, k, w)
__global__ __launch_bounds__(TPB) void aa_softmax_kernel(const float* __restrict__ S, const float* __restrict__ A, int NK, int K, int V,
                                                         float* __restrict__ P, float* __restrict__ Aeff) {
  const int g = blockIdx.x * TPB + threadIdx.x, nk = g / V, w = g - nk * V;
  if (nk >= NK) return;
  const int64_t at = (int64_t)nk * V * V + w;
  const float* s = S + at;
  const float* a = A + (nk % K) * V * V + w;
  float m = s[0];
  for (int v = 1; v < V; ++v) m = fmaxf(m, s[v * V]);
  float sum = 0.f;
  for (int v = 0; v < V; ++v) sum += expf(s[v * V] - m);
  for (int v = 0; v < V; ++v) {
    const float p = expf(s[v * V] - m) / sum;
    P[at + v * V] = p;
    Aeff[at + v * V] = a[v * V] + p;
  }
}

// the same walk: g = sum_v P dA_eff (fp64), dS = P (dA_eff - g)
__global__ __launch_bounds__(TPB) void aa_softmax_bwd_kernel(const float* __restrict__ P, const float* __restrict__ dAeff, int NK, int V,
                                                             float* __restrict__ dS) {
  const int g = blockIdx.x * TPB + threadIdx.x, nk = g / V, w = g - nk * V;
  if (nk >= NK) return;
  const int64_t at = (int64_t)nk * V * V + w;
  const float* p = P + at;
  const float* d = dAeff + at;
  double sum = 0.0;
  for (int v = 0; v < V; ++v) sum += (double)p[v * V] * (double)d[v * V];
  const float gw = (float)sum;
  for (int v = 0; v < V; ++v) dS[at + v * V] = p[v * V] * (d[v * V] - gw);
}

// grid ceil(K V V / 256): dA[i] = sum_n dA_eff[n][i], in sample order, fp64
__global__ __launch_bounds__(TPB) void aa_dadj_kernel(const float* __restrict__ dAeff, int N, int kvv, float* __restrict__ dA) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= kvv) return;
  double sum = 0.0;
#pragma unroll 4
  for (int n = 0; n < N; ++n) sum += (double)dAeff[(int64_t)n * kvv + i];
  dA[i] = (float)sum;
}

// grid (N K, chunks); tile = (channel tile / tpe, frames 32 (tile % tpe) ..); wave w owns tiles 4 chunk + w, + 4 chunks, ..
__global__ __launch_bounds__(TPB) void aa_dembed_kernel(const float* __restrict__ dS, const float* __restrict__ theta, const float* __restrict__ phi,
                                                        int64_t ld, int K, int Ce, int T, int V, int tpe, int ntiles, float c,
                                                        float* __restrict__ dtheta, float* __restrict__ dphi, int64_t ldd) {
  __shared__ float st[4][2][DE_TR * 32];       // per wave: its tile of theta and of phi as they lie in memory, [frame][V]; zero past the tile
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lo = lane & 31, hi = lane >> 5;
  const int nk = blockIdx.x, n = nk / K, k = nk - n * K;
  const float* ds = dS + (int64_t)nk * V * V;
  float bt[16], bp[16];                        // step i, this lane's j = 2 i + hi: dS[lo][j] (dtheta sums over w = j), dS[j][lo] (dphi over v = j)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = 2 * i + hi;
    const bool ok = lo < V && j < V;
    bt[i] = ok ? ds[lo * V + j] : 0.f;
    bp[i] = ok ? ds[j * V + lo] : 0.f;
  }
  float rt[16], rp[16];                        // the tile in flight: element lane + 64 m of its run of rows * V floats
  auto fetch = [&](int tile) {
    int cnt = 0;
    int64_t at = 0;
    if (tile < ntiles) {
      const int e = tile / tpe, t0 = (tile - e * tpe) * DE_TR, rows = T - t0 < DE_TR ? T - t0 : DE_TR;
      cnt = rows * V;
      at = ((int64_t)k * Ce + e) * ld + (int64_t)n * T * V + (int64_t)t0 * V;
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int idx = lane + 64 * m;
      rt[m] = idx < cnt ? theta[at + idx] : 0.f;
      rp[m] = idx < cnt ? phi[at + idx] : 0.f;
    }
  };
  // the trip count is the workgroup's, not the wave's: every wave meets every barrier
  const int step = gridDim.y * 4;
  fetch(blockIdx.y * 4 + w);
  for (int base = blockIdx.y * 4; base < ntiles; base += step) {
    const int tile = base + w;
    __syncthreads();                           // the previous tile's operands have been read
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      st[w][0][lane + 64 * m] = rt[m];
      st[w][1][lane + 64 * m] = rp[m];
    }
    __syncthreads();
    if (base + step < ntiles) fetch(tile + step);
    float at[16], ap[16];                      // this lane's frame lo of the tile: phi[.][j] for dtheta, theta[.][j] for dphi
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = 2 * i + hi;
      at[i] = j < V ? st[w][1][lo * V + j] : 0.f;
      ap[i] = j < V ? st[w][0][lo * V + j] : 0.f;
    }
    f32x16 acct, accp;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acct[reg] = 0.f, accp[reg] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acct = __builtin_amdgcn_mfma_f32_32x32x2f32(at[i], bt[i], acct, 0, 0, 0);
      accp = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[i], bp[i], accp, 0, 0, 0);
    }
    if (tile >= ntiles) continue;              // (wave-uniform; no barrier is skipped: the next one is at the head of the loop)
    const int e = tile / tpe, t0 = (tile - e * tpe) * DE_TR, rows = T - t0 < DE_TR ? T - t0 : DE_TR;
    const int64_t out = ((int64_t)k * Ce + e) * ldd + (int64_t)n * T * V + (int64_t)t0 * V + lo;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = mfma_row(reg, hi);
      if (lo < V && r < rows) {
        dtheta[out + r * V] = acct[reg] * c;
        dphi[out + r * V] = accp[reg] * c;
      }
    }
  }
}

inline int aa_pairs(int T) { return (T + 1) / 2; }

// slabs of the similarity: about SIM_SLAB_STEPS steps each, at most SIM_SLAB_MAX -- (Ce, T) alone
inline int aa_slabs(int Ce, int T) {
  const int64_t nsteps = (int64_t)Ce * aa_pairs(T);
  const int64_t s = (nsteps + SIM_SLAB_STEPS - 1) / SIM_SLAB_STEPS;
  return s > SIM_SLAB_MAX ? SIM_SLAB_MAX : s < 1 ? 1 : (int)s;
}

// every limit, before any launch; Ce = T = 1 for the entry points that see neither
int aa_dims(const char* who, int N, int K, int Ce, int T, int V) {
  SAR_REQUIRE(N >= 1 && K >= 1 && Ce >= 1 && T >= 1 && V >= 1, "%s: need N, K, Ce, T, V >= 1 (got %d, %d, %d, %d, %d)", who, N, K, Ce, T, V);
  if (V > AA_VMAX || K > AA_KMAX || (int64_t)K * Ce > AA_EMAX || (int64_t)N * T * V >= ((int64_t)1 << 22) || (int64_t)N * K > 65535) {
    sar_set_error("%s: built for V <= %d, K <= %d, K * Ce <= %d, N * T * V < 2^22 and N * K <= 65535 (got N = %d, K = %d, Ce = %d, T = %d, V = %d)",
                  who, AA_VMAX, AA_KMAX, AA_EMAX, N, K, Ce, T, V);
    return SAR_E_UNSUP;
  }
  return 0;
}

}  // namespace

#define AA_DIMS(name, Ce, T) \
  if (int rc__ = aa_dims(name, N, K, Ce, T, V)) return rc__
#define AA_LD(name, ld)                                                                                                              \
  SAR_REQUIRE((ld) >= (int64_t)N * T * V && (ld) < ((int64_t)1 << 31), "%s: a [K Ce][ld] matrix needs N T V <= ld < 2^31 (got %lld)", name, \
              (long long)(ld))

extern "C" int sar_adjattn_sim_slabs(int Ce, int T, int V) {
  if (int rc = aa_dims("sar_adjattn_sim_slabs", 1, 1, Ce, T, V)) return rc;
  return aa_slabs(Ce, T);
}

extern "C" int sar_adjattn_sim_f32(const float* theta, const float* phi, int64_t ld, int N, int K, int Ce, int T, int V, float* S, float* slab,
                                   int nslab, sar_stream_t s) {
  AA_DIMS("sar_adjattn_sim_f32", Ce, T);
  SAR_REQUIRE(theta && phi && S, "sar_adjattn_sim_f32: null operand");
  SAR_REQUIRE(nslab == aa_slabs(Ce, T), "sar_adjattn_sim_f32: nslab must be sar_adjattn_sim_slabs(Ce, T, V) = %d (got %d)", aa_slabs(Ce, T), nslab);
  SAR_REQUIRE(nslab == 1 || slab, "sar_adjattn_sim_f32: %d slabs need a slab buffer of %d * N K V V floats", nslab, nslab);
  SAR_REQUIRE(S != theta && S != phi && (nslab == 1 || (slab != theta && slab != phi && slab != S)), "sar_adjattn_sim_f32: an output is an input");
  AA_LD("sar_adjattn_sim_f32", ld);
  const int npairs = aa_pairs(T), nsteps = Ce * npairs, sps = (nsteps + nslab - 1) / nslab;
  const int64_t size = (int64_t)N * K * V * V;
  const double denom = (double)Ce * T;
  hipLaunchKernelGGL(aa_sim_kernel, dim3(N * K, nslab), dim3(TPB), 0, as_stream(s), theta, phi, ld, K, Ce, T, V, npairs, sps, nsteps,
                     nslab == 1 ? denom : 1.0, nslab == 1 ? S : slab, size);
  SAR_LAUNCH_CHECK("sar_adjattn_sim_f32");
  if (nslab > 1) {
    hipLaunchKernelGGL(aa_sim_finish_kernel, dim3((unsigned)((size + TPB - 1) / TPB)), dim3(TPB), 0, as_stream(s), slab, nslab, size, size, denom, S);
    SAR_LAUNCH_CHECK("sar_adjattn_sim_f32");
  }
  return 0;
}

extern "C" int sar_adjattn_softmax_f32(const float* S, const float* A, int N, int K, int V, float* P, float* A_eff, sar_stream_t s) {
  AA_DIMS("sar_adjattn_softmax_f32", 1, 1);
  SAR_REQUIRE(S && A && P && A_eff, "sar_adjattn_softmax_f32: null operand");
  SAR_REQUIRE(P != S && P != A && A_eff != S && A_eff != A && A_eff != P, "sar_adjattn_softmax_f32: an output is an input, or P is A_eff");
  hipLaunchKernelGGL(aa_softmax_kernel, dim3((N * K * V + TPB - 1) / TPB), dim3(TPB), 0, as_stream(s), S, A, N * K, K, V, P, A_eff);
  SAR_LAUNCH_CHECK("sar_adjattn_softmax_f32");
  return 0;
}

extern "C" int sar_adjattn_softmax_bwd_f32(const float* P, const float* dA_eff, int N, int K, int V, float* dS, float* dA, sar_stream_t s) {
  AA_DIMS("sar_adjattn_softmax_bwd_f32", 1, 1);
  SAR_REQUIRE(P && dA_eff && dS, "sar_adjattn_softmax_bwd_f32: null operand");
  SAR_REQUIRE(dS != P && dS != dA_eff && dA != P && dA != dA_eff && dA != dS, "sar_adjattn_softmax_bwd_f32: an output is an input, or dA is dS");
  hipLaunchKernelGGL(aa_softmax_bwd_kernel, dim3((N * K * V + TPB - 1) / TPB), dim3(TPB), 0, as_stream(s), P, dA_eff, N * K, V, dS);
  SAR_LAUNCH_CHECK("sar_adjattn_softmax_bwd_f32");
  if (dA) {
    hipLaunchKernelGGL(aa_dadj_kernel, dim3((K * V * V + TPB - 1) / TPB), dim3(TPB), 0, as_stream(s), dA_eff, N, K * V * V, dA);
    SAR_LAUNCH_CHECK("sar_adjattn_softmax_bwd_f32");
  }
  return 0;
}

extern "C" int sar_adjattn_dembed_f32(const float* dS, const float* theta, const float* phi, int64_t ld, int N, int K, int Ce, int T, int V,
                                      float* dtheta, float* dphi, int64_t ld_d, sar_stream_t s) {
  AA_DIMS("sar_adjattn_dembed_f32", Ce, T);
  SAR_REQUIRE(dS && theta && phi && dtheta && dphi, "sar_adjattn_dembed_f32: null operand");
  SAR_REQUIRE(dtheta != dphi && dtheta != theta && dtheta != phi && dtheta != dS && dphi != theta && dphi != phi && dphi != dS,
              "sar_adjattn_dembed_f32: an output is an input, or dtheta is dphi");
  AA_LD("sar_adjattn_dembed_f32", ld);
  AA_LD("sar_adjattn_dembed_f32", ld_d);
  const int tpe = (T + DE_TR - 1) / DE_TR, ntiles = Ce * tpe;
  int chunks = (ntiles + DE_TILES - 1) / DE_TILES;
  if (chunks > DE_CHUNK_MAX) chunks = DE_CHUNK_MAX;
  hipLaunchKernelGGL(aa_dembed_kernel, dim3(N * K, chunks), dim3(TPB), 0, as_stream(s), dS, theta, phi, ld, K, Ce, T, V, tpe, ntiles,
                     (float)(1.0 / ((double)Ce * T)), dtheta, dphi, ld_d);
  SAR_LAUNCH_CHECK("sar_adjattn_dembed_f32");
  return 0;
}
