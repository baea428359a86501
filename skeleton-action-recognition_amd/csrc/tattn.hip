// tattn.hip -- TemporalAttention(num_hidden), the per-frame gate of models/stgcn.py:67-85, fp32, forward and backward.
// x (N, C, T, V); rows r = n T + t; the first Dense contracts over the K = V C features f[r, v C + c] = x[n, c, t, v] of a frame:
//
//   H1[j][r] = act(sum_{c,v} kernel_1[v C + c][j] x[n, c, t, v] + bias_1[j])      (ReLU, or sigmoid where the stack is one layer deep)
//   ... layers 2 .. L are the library's 1x1 products on the [units][N T] matrices ...     a[r] = sigmoid(z_L[r])
//   out[n, c, t, v] = x[n, c, t, v] a[r]
//   dz_L[r] = (sum_{c,v} dout x) a (1 - a)        dkernel_1[v C + c][j] = sum_r x[n, c, t, v] dz_1[j][r]      dbias_1[j] = sum_r dz_1[j][r]
//   dx[n, c, t, v] = dout[n, c, t, v] a[r] + sum_j kernel_1[v C + c][j] dz_1[j][r]
//
// Addressing: element (n, c, t, v) of x / out / dout / dx is at n s_n + c s_c + t V + v (csrc/gpool.hip): NCHW tensors and the engines'
// CN matrices [C][ld] are the same kernels, and NO packed, transposed or feature-major copy of x or dout is made.  The run of T V
// floats of one (n, c) is contiguous and aligned to 4 bytes only (V = 25: 100-byte rows): every access is one dword of one lane
// under a predicate.  The three products run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation), and each walks
// K or its rows in an order that makes the operand a contiguous run of x:
//
//   score   a workgroup owns 64 consecutive rows and all units.  K is walked CHANNEL-major: one step = the (up to 32) joints of one
//           channel, whose 64 x V floats are 64 runs of V (one run of 64 V inside a sample) and whose weight rows are v C + c.  Both
//           operands of a step go global -> registers -> LDS while the previous step's MFMAs run (two LDS stages, one barrier per
//           step).  Wave w owns row half w & 1 and the 32-unit blocks (w >> 1), (w >> 1) + 2.
//   wgrad   grid (groups of 4 channels, slabs).  Wave w owns channel 4 g + w and the whole [V][units] block of dkernel_1 for it; the
//           reduction index is the row, walked in tiles of 32 frames of ONE sample (a contiguous run of 32 V floats per channel,
//           frames past T are zero).  dz_1's tile [units][32] is shared by the four waves through LDS.  The tiles are cut into
//           sar_tattn_wgrad_slabs(N, C, T, V) slabs -- a function of the shape alone --, each slab writes its own [V C units + units]
//           partial (every element), and sar_slab_reduce_f32 adds the slabs in order.  dbias_1 is summed per unit in row order by
//           the workgroups of group 0.
//   dx      grid (channels, row blocks).  kernel_1's rows of the channel sit in LDS as [units][V]; a wave owns tiles of 32 frames of
//           one sample, reads dz_1 along the row index (coalesced) and writes dx = dout a + product once, from the accumulators.
//   scale / dscore walk x as csrc/gpool.hip does: lane -> (frame of the step, joint), fixed for the whole walk.  dscore keeps one
//           fp32 fmaf chain per lane over the channels, and one lane per frame adds the V chains in joint order in fp64.
// No atomics; every sum has one fixed order; a row's result is computed from the row's own data by the same sequence of
// operations wherever it sits in the batch: bitwise deterministic, and a sample's out / dx do not depend on the rest of the batch.
#include "sar_common.h"

namespace {

constexpr int TPB = 256;
constexpr int TA_UMAX = SAR_TATTN_UMAX, TA_VMAX = SAR_TATTN_VMAX;
constexpr int SC_TR = 64;                     // rows of a score workgroup
constexpr int SC_XS = SC_TR + 1;              // LDS row stride of its x stage [joint][row]: the transposing write is conflict-free
constexpr int SC_KV = 32;                     // joints per K step
constexpr int TR = 32;                        // frames of a wgrad / dx tile
constexpr int WG_DS = TR + 1;                 // LDS row stride of wgrad's dz stage [unit][frame]
constexpr int WG_CH = 4;                      // channels of a wgrad workgroup, one per wave
constexpr int EW_U = 8;                       // steps of the scale walk per workgroup

struct ta_view {
  const float* p;
  int64_t sn, sc;
};
struct ta_wview {
  float* p;
  int64_t sn, sc;
};

__device__ __forceinline__ float ta_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// grid ceil(N T / 64); Q = 32-unit blocks per wave (1: units <= 64, 2: units <= 128)
template <int Q>
__global__ __launch_bounds__(TPB) void ta_score_kernel(const ta_view x, const float* __restrict__ W, const float* __restrict__ bias, int N,
                                                       int C, int T, int V, int u, int act, float* __restrict__ h, int64_t ld) {
  __shared__ float ws[2][SC_KV * TA_UMAX];    // [joint of the step][unit]
  __shared__ float xs[2][SC_KV * SC_XS];      // [joint of the step][row]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lo = lane & 31, hi = lane >> 5;
  const int R = N * T, r0 = blockIdx.x * SC_TR;
  const int nvc = (V + SC_KV - 1) / SC_KV, kvm = V < SC_KV ? V : SC_KV, kvp = (kvm + 1) & ~1;
  const int nxs = (SC_TR * kvp + TPB - 1) / TPB, nws = kvp >> 1;
  // this lane's share of a step's x: element e = (row e / kvp, joint e % kvp) of the 64 x kvp grid; -1 = not in the tensor
  int64_t xoff[8];
  int xl[8], xv[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int e = tid + TPB * m, rr = e / kvp, vv = e - rr * kvp, r = r0 + rr;
    xl[m] = rr < SC_TR ? vv * SC_XS + rr : -1;
    xv[m] = vv;
    xoff[m] = -1;
    if (rr < SC_TR && r < R) {
      const int n = r / T, t = r - n * T;
      xoff[m] = n * x.sn + (int64_t)t * V + vv;
    }
  }
  const int wi = tid & (TA_UMAX - 1), wk = tid >> 7;        // this lane's unit, and its joint of the step: wk + 2 m
  float xr[8], wr[16];
  auto fetch = [&](int c, int v0) {
    const float* xp = x.p + c * x.sc + v0;
#pragma unroll
    for (int m = 0; m < 8; ++m)
      if (m < nxs) xr[m] = (xoff[m] >= 0 && v0 + xv[m] < V) ? xp[xoff[m]] : 0.f;
#pragma unroll
    for (int m = 0; m < 16; ++m)
      if (m < nws) {
        const int v = v0 + wk + 2 * m;
        wr[m] = (wi < u && v < V) ? W[((int64_t)v * C + c) * u + wi] : 0.f;
      }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
      if (m < nxs && xl[m] >= 0) xs[b][xl[m]] = xr[m];
#pragma unroll
    for (int m = 0; m < 16; ++m)
      if (m < nws) ws[b][(wk + 2 * m) * TA_UMAX + wi] = wr[m];
  };
  const int jb = w & 1, ib0 = w >> 1;        // a unit block past the units multiplies zeros (ws is zero there)
  f32x16 acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[q][reg] = 0.f;
  const int nsteps = C * nvc;
  fetch(0, 0);
  stash(0);
  __syncthreads();
  int c = 0, vc = 0;
  for (int s = 0; s < nsteps; ++s) {
    const int b = s & 1, kv = V - vc * SC_KV < SC_KV ? V - vc * SC_KV : SC_KV, kend = (kv + 1) & ~1;
    int cn = c, vn = vc + 1;
    if (vn == nvc) vn = 0, ++cn;
    if (s + 1 < nsteps) fetch(cn, vn * SC_KV);
    const float* xb = xs[b] + hi * SC_XS + jb * 32 + lo;
    const float* wb = ws[b] + hi * TA_UMAX + ib0 * 32 + lo;
    for (int k0 = 0; k0 < kend; k0 += 2) {
      const float bv = xb[k0 * SC_XS];
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[k0 * TA_UMAX + q * 64], bv, acc[q], 0, 0, 0);
    }
    if (s + 1 < nsteps) stash(b ^ 1);       // the other stage: every wave left it before the barrier that ended step s - 1
    __syncthreads();
    c = cn, vc = vn;
  }
  const int r = r0 + jb * 32 + lo;
  if (r >= R) return;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int ib = ib0 + 2 * q;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = ib * 32 + mfma_row(reg, hi);
      if (i < u) {
        const float z = acc[q][reg] + bias[i];
        h[i * ld + r] = act == SAR_TATTN_SIGMOID ? ta_sigmoid(z) : fmaxf(z, 0.f);
      }
    }
  }
}

// grid N C ceil(T / (EW_U G)); lane -> (tt, v)
__global__ __launch_bounds__(TPB) void ta_scale_kernel(const ta_view x, const float* __restrict__ a, int C, int T, int V, int tch,
                                                       const ta_wview out) {
  const int G = TPB / V, tt = threadIdx.x / V, v = threadIdx.x - tt * V;
  if (tt >= G) return;
  const int nc = blockIdx.x / tch, ch = blockIdx.x - nc * tch, n = nc / C, c = nc - n * C;
  const float* xr = x.p + n * x.sn + c * x.sc + v;
  float* o = out.p + n * out.sn + c * out.sc + v;
  const float* ar = a + (int64_t)n * T;
#pragma unroll
  for (int it = 0; it < EW_U; ++it) {
    const int t = (ch * EW_U + it) * G + tt;
    if (t < T) o[t * V] = xr[t * V] * ar[t];
  }
}

// grid N ceil(T / G); lane -> (tt, v): one fmaf chain over the channels per lane, then one lane per frame adds the joints in order
__global__ __launch_bounds__(TPB) void ta_dscore_kernel(const ta_view x, const ta_view dout, const float* __restrict__ a, int C, int T, int V,
                                                        int tch, float* __restrict__ dz) {
  __shared__ float red[TPB];
  const int G = TPB / V, tt = threadIdx.x / V, v = threadIdx.x - tt * V;
  const int n = blockIdx.x / tch, ch = blockIdx.x - n * tch, t = ch * G + tt;
  float acc = 0.f;
  if (tt < G && t < T) {
    const float* xr = x.p + n * x.sn + (int64_t)t * V + v;
    const float* dr = dout.p + n * dout.sn + (int64_t)t * V + v;
#pragma unroll 8
    for (int c = 0; c < C; ++c) acc = fmaf(dr[c * dout.sc], xr[c * x.sc], acc);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  const int t1 = ch * G + threadIdx.x;
  if (threadIdx.x < G && t1 < T) {
    double s = 0.0;
    for (int j = 0; j < V; ++j) s += (double)red[threadIdx.x * V + j];
    const float av = a[(int64_t)n * T + t1];
    dz[(int64_t)n * T + t1] = (float)s * av * (1.f - av);
  }
}

// grid (ceil(C / 4), slabs); tile ti = (sample ti / tps, frames 32 (ti % tps) ..).  NVB = 32-joint blocks, NJB = 32-unit blocks
template <int NVB, int NJB>
__global__ __launch_bounds__(TPB) void ta_wgrad_kernel(const ta_view x, const float* __restrict__ dz, int64_t ld, int C, int T, int V, int u,
                                                       int tps, int ntiles, int tpsl, float* __restrict__ slab, int64_t slab_stride) {
  constexpr int XS = TR * 32 * NVB, NX = XS / 64, ND = 4 * NJB;
  __shared__ float xs[WG_CH][XS];             // per wave: its channel's [frame][joint] run, as it lies in memory
  __shared__ float dzs[32 * NJB * WG_DS];     // [unit][frame]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lo = lane & 31, hi = lane >> 5;
  const int c = blockIdx.x * WG_CH + w;
  const bool cl = c < C;
  const int tile0 = blockIdx.y * tpsl, tile1 = tile0 + tpsl < ntiles ? tile0 + tpsl : ntiles;
  f32x16 acc[NVB][NJB];
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc[vb][jb][reg] = 0.f;
  float bsum = 0.f;
  float xr[NX], dr[ND];
  const int dj = tid >> 5, drr = tid & 31;    // this lane's unit dj + 8 m and frame of the dz stage
  auto fetch = [&](int ti) {
    const int n = ti / tps, t0 = (ti - n * tps) * TR, rows = T - t0 < TR ? T - t0 : TR, cnt = cl ? rows * V : 0;
    const float* xp = x.p + n * x.sn + (cl ? c : 0) * x.sc + (int64_t)t0 * V;
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      const int idx = lane + 64 * m;
      xr[m] = idx < cnt ? xp[idx] : 0.f;
    }
    const float* dp = dz + (int64_t)n * T + t0 + drr;
#pragma unroll
    for (int m = 0; m < ND; ++m) {
      const int j = dj + 8 * m;
      dr[m] = (j < u && drr < rows) ? dp[j * ld] : 0.f;
    }
  };
  if (tile0 < tile1) fetch(tile0);
  for (int ti = tile0; ti < tile1; ++ti) {
    __syncthreads();                          // the previous tile's operands have been read
#pragma unroll
    for (int m = 0; m < NX; ++m) xs[w][lane + 64 * m] = xr[m];
#pragma unroll
    for (int m = 0; m < ND; ++m) dzs[(dj + 8 * m) * WG_DS + drr] = dr[m];
    __syncthreads();
    if (ti + 1 < tile1) fetch(ti + 1);
    const float* xa = xs[w] + hi * V + lo;
    const float* db = dzs + lo * WG_DS + hi;
#pragma unroll 8
    for (int k0 = 0; k0 < TR; k0 += 2) {
      float av[NVB], bv[NJB];
#pragma unroll
      for (int vb = 0; vb < NVB; ++vb) av[vb] = vb * 32 + lo < V ? xa[k0 * V + vb * 32] : 0.f;
#pragma unroll
      for (int jb = 0; jb < NJB; ++jb) bv[jb] = db[jb * 32 * WG_DS + k0];
#pragma unroll
      for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) acc[vb][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[vb], bv[jb], acc[vb][jb], 0, 0, 0);
    }
    if (blockIdx.x == 0 && tid < u)
      for (int rr = 0; rr < TR; ++rr) bsum += dzs[tid * WG_DS + rr];
  }
  float* o = slab + blockIdx.y * slab_stride;
  if (blockIdx.x == 0 && tid < u) o[(int64_t)V * C * u + tid] = bsum;
  if (!cl) return;
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      const int j = jb * 32 + lo;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int v = vb * 32 + mfma_row(reg, hi);
        if (v < V && j < u) o[((int64_t)v * C + c) * u + j] = acc[vb][jb][reg];
      }
    }
}

// grid (C, row blocks); a wave owns tiles tile0 + w, tile0 + w + 4, ..  NVB = 32-joint blocks, NJB = 32-unit blocks
template <int NVB, int NJB>
__global__ __launch_bounds__(TPB) void ta_dx_kernel(const ta_view dout, const float* __restrict__ a, const float* __restrict__ W,
                                                    const float* __restrict__ dz, int64_t ld, int C, int T, int V, int u, int tps,
                                                    int ntiles, int tpb, const ta_wview dx) {
  constexpr int VP = 32 * NVB, KP = 32 * NJB, KS = 16 * NJB;
  __shared__ float ws[KP * VP];               // [unit][joint]; units past u and joints past V are zero
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lo = lane & 31, hi = lane >> 5;
  const int c = blockIdx.x;
  for (int e = tid; e < KP * VP; e += TPB) {
    const int v = e / KP, k = e - v * KP;
    ws[k * VP + v] = (k < u && v < V) ? W[((int64_t)v * C + c) * u + k] : 0.f;
  }
  __syncthreads();
  const int tile0 = blockIdx.y * tpb, tile1 = tile0 + tpb < ntiles ? tile0 + tpb : ntiles;
  const float* wb = ws + hi * VP + lo;
  for (int ti = tile0 + w; ti < tile1; ti += 4) {
    const int n = ti / tps, t0 = (ti - n * tps) * TR, rows = T - t0 < TR ? T - t0 : TR;
    const int64_t r0 = (int64_t)n * T + t0;
    const float* dp = dz + r0 + lo;
    float av[KS];                             // this lane's operands of every K step, all in flight at once
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const int k = 2 * i + hi;
      av[i] = (k < u && lo < rows) ? dp[k * ld] : 0.f;
    }
    f32x16 acc[NVB];
#pragma unroll
    for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc[vb][reg] = 0.f;
#pragma unroll
    for (int i = 0; i < KS; ++i)
#pragma unroll
      for (int vb = 0; vb < NVB; ++vb) acc[vb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], wb[2 * i * VP + vb * 32], acc[vb], 0, 0, 0);
    const float* dr = dout.p + n * dout.sn + c * dout.sc + (int64_t)t0 * V;
    float* o = dx.p + n * dx.sn + c * dx.sc + (int64_t)t0 * V;
#pragma unroll
    for (int vb = 0; vb < NVB; ++vb) {
      const int v = vb * 32 + lo;
      if (v >= V) continue;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = mfma_row(reg, hi);
        if (row < rows) o[row * V + v] = fmaf(dr[row * V + v], a[r0 + row], acc[vb][reg]);
      }
    }
  }
}

// grid (ceil(n / 256), rows)
__global__ __launch_bounds__(TPB) void ta_act_kernel(float* __restrict__ z, int64_t ld, int64_t n, int act) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  float* p = z + blockIdx.y * ld + i;
  *p = act == SAR_TATTN_SIGMOID ? ta_sigmoid(*p) : fmaxf(*p, 0.f);
}

__global__ __launch_bounds__(TPB) void ta_dact_kernel(const float* __restrict__ h, int64_t ld_h, float* __restrict__ dh, int64_t ld_dh, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (!(h[blockIdx.y * ld_h + i] > 0.f)) dh[blockIdx.y * ld_dh + i] = 0.f;
}

inline int ta_tiles_per_sample(int T) { return (T + TR - 1) / TR; }

// slabs of the first layer's weight gradient: about 512 workgroups, at least 4 tiles a slab, at most 64 slabs -- the shape alone
inline int ta_slabs(int N, int C, int T) {
  const int64_t ntiles = (int64_t)N * ta_tiles_per_sample(T);
  const int groups = (C + WG_CH - 1) / WG_CH;
  int64_t s = (512 + groups - 1) / groups;
  if (s > (ntiles + 3) / 4) s = (ntiles + 3) / 4;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

// every limit, before any launch
int ta_dims(const char* who, int N, int C, int T, int V, int u) {
  SAR_REQUIRE(N >= 1 && C >= 1 && T >= 1 && V >= 1 && u >= 1, "%s: need N, C, T, V, units >= 1 (got %d, %d, %d, %d, units %d)", who, N, C, T, V, u);
  const int64_t nt = (int64_t)N * T;
  if (u > TA_UMAX || V > TA_VMAX || nt >= ((int64_t)1 << 22) || nt * ((int64_t)C * V) >= ((int64_t)1 << 31)) {
    sar_set_error("%s: built for units <= %d, V <= %d, N * T < 2^22 and N * C * T * V < 2^31 (got N = %d, C = %d, T = %d, V = %d, units %d)", who,
                  TA_UMAX, TA_VMAX, N, C, T, V, u);
    return SAR_E_UNSUP;
  }
  return 0;
}

// the runs of W floats of a strided (N, C, T, V) tensor lie inside it and do not overlap (csrc/gpool.hip)
bool ta_strides_ok(int64_t sn, int64_t sc, int N, int C, int64_t W) {
  const int64_t lim = (int64_t)1 << 31;
  if (sn < 1 || sc < 1 || sn >= lim || sc >= lim) return false;
  const bool nchw = sc >= W && (C == 1 || N == 1 || sn >= (int64_t)C * sc), cn = sn >= W && (N == 1 || C == 1 || sc >= (int64_t)N * sn);
  return (nchw || cn) && (N - 1) * sn + (C - 1) * sc + W <= lim;
}

}  // namespace

// the instantiation for V joints (one or two blocks of 32) and `units` (one to four blocks of 32)
#define TA_PICK2(kern, nvb, units) \
  ((units) <= 32 ? kern<nvb, 1> : (units) <= 64 ? kern<nvb, 2> : (units) <= 96 ? kern<nvb, 3> : kern<nvb, 4>)
#define TA_PICK(kern, V, units) ((V) <= 32 ? TA_PICK2(kern, 1, units) : TA_PICK2(kern, 2, units))
#define TA_DIMS(name, u)                                \
  if (int rc__ = ta_dims(name, N, C, T, V, u)) return rc__
#define TA_STRIDES(name, sn, sc)                                                                                                       \
  SAR_REQUIRE(ta_strides_ok(sn, sc, N, C, (int64_t)T * V), "%s: strides (%lld, %lld) do not describe a (N, C, T, V) tensor", name, \
              (long long)(sn), (long long)(sc))
#define TA_LD(name, ld)                                                                                                         \
  SAR_REQUIRE((ld) >= (int64_t)N * T && (ld) < ((int64_t)1 << 31), "%s: a [units][N T] matrix needs N T <= ld < 2^31 (got %lld)", name, \
              (long long)(ld))

extern "C" int sar_tattn_score_f32(const float* x, int64_t s_n, int64_t s_c, const float* kernel, const float* bias, int N, int C, int T,
                                   int V, int units, int act, float* h, int64_t ld_h, sar_stream_t s) {
  TA_DIMS("sar_tattn_score_f32", units);
  SAR_REQUIRE(x && kernel && bias && h, "sar_tattn_score_f32: null operand");
  SAR_REQUIRE(act == SAR_TATTN_RELU || act == SAR_TATTN_SIGMOID, "sar_tattn_score_f32: act must be SAR_TATTN_RELU or SAR_TATTN_SIGMOID (got %d)", act);
  TA_STRIDES("sar_tattn_score_f32", s_n, s_c);
  TA_LD("sar_tattn_score_f32", ld_h);
  const auto k = units <= 64 ? ta_score_kernel<1> : ta_score_kernel<2>;
  hipLaunchKernelGGL(k, dim3((N * T + SC_TR - 1) / SC_TR), dim3(TPB), 0, as_stream(s), ta_view{x, s_n, s_c}, kernel, bias, N, C, T, V, units, act, h,
                     ld_h);
  SAR_LAUNCH_CHECK("sar_tattn_score_f32");
  return 0;
}

extern "C" int sar_tattn_scale_f32(const float* x, int64_t s_n, int64_t s_c, const float* a, int N, int C, int T, int V, float* out,
                                   int64_t o_sn, int64_t o_sc, sar_stream_t s) {
  TA_DIMS("sar_tattn_scale_f32", 1);
  SAR_REQUIRE(x && a && out, "sar_tattn_scale_f32: null operand");
  TA_STRIDES("sar_tattn_scale_f32", s_n, s_c);
  TA_STRIDES("sar_tattn_scale_f32", o_sn, o_sc);
  const int G = TPB / V, tch = (T + EW_U * G - 1) / (EW_U * G);
  hipLaunchKernelGGL(ta_scale_kernel, dim3((unsigned)((int64_t)N * C * tch)), dim3(TPB), 0, as_stream(s), ta_view{x, s_n, s_c}, a, C, T, V, tch,
                     ta_wview{out, o_sn, o_sc});
  SAR_LAUNCH_CHECK("sar_tattn_scale_f32");
  return 0;
}

extern "C" int sar_tattn_dscore_f32(const float* x, int64_t s_n, int64_t s_c, const float* dout, int64_t d_sn, int64_t d_sc, const float* a,
                                    int N, int C, int T, int V, float* dz, sar_stream_t s) {
  TA_DIMS("sar_tattn_dscore_f32", 1);
  SAR_REQUIRE(x && dout && a && dz, "sar_tattn_dscore_f32: null operand");
  TA_STRIDES("sar_tattn_dscore_f32", s_n, s_c);
  TA_STRIDES("sar_tattn_dscore_f32", d_sn, d_sc);
  const int G = TPB / V, tch = (T + G - 1) / G;
  hipLaunchKernelGGL(ta_dscore_kernel, dim3((unsigned)((int64_t)N * tch)), dim3(TPB), 0, as_stream(s), ta_view{x, s_n, s_c},
                     ta_view{dout, d_sn, d_sc}, a, C, T, V, tch, dz);
  SAR_LAUNCH_CHECK("sar_tattn_dscore_f32");
  return 0;
}

extern "C" int sar_tattn_wgrad_slabs(int N, int C, int T, int V) {
  if (int rc = ta_dims("sar_tattn_wgrad_slabs", N, C, T, V, 1)) return rc;
  return ta_slabs(N, C, T);
}

extern "C" int sar_tattn_wgrad_f32(const float* x, int64_t s_n, int64_t s_c, const float* dz, int64_t ld_dz, int N, int C, int T, int V,
                                   int units, float* slab, int nslab, sar_stream_t s) {
  TA_DIMS("sar_tattn_wgrad_f32", units);
  SAR_REQUIRE(x && dz && slab, "sar_tattn_wgrad_f32: null operand");
  SAR_REQUIRE(nslab == ta_slabs(N, C, T), "sar_tattn_wgrad_f32: nslab must be sar_tattn_wgrad_slabs(N, C, T, V) = %d (got %d)", ta_slabs(N, C, T),
              nslab);
  TA_STRIDES("sar_tattn_wgrad_f32", s_n, s_c);
  TA_LD("sar_tattn_wgrad_f32", ld_dz);
  const int tps = ta_tiles_per_sample(T), ntiles = N * tps, tpsl = (ntiles + nslab - 1) / nslab;
  const auto k = TA_PICK(ta_wgrad_kernel, V, units);
  hipLaunchKernelGGL(k, dim3((C + WG_CH - 1) / WG_CH, nslab), dim3(TPB), 0, as_stream(s), ta_view{x, s_n, s_c}, dz, ld_dz, C, T, V,
                     units, tps, ntiles, tpsl, slab, (int64_t)V * C * units + units);
  SAR_LAUNCH_CHECK("sar_tattn_wgrad_f32");
  return 0;
}

extern "C" int sar_tattn_dx_f32(const float* dout, int64_t d_sn, int64_t d_sc, const float* a, const float* kernel, const float* dz,
                                int64_t ld_dz, int N, int C, int T, int V, int units, float* dx, int64_t g_sn, int64_t g_sc, sar_stream_t s) {
  TA_DIMS("sar_tattn_dx_f32", units);
  SAR_REQUIRE(dout && a && kernel && dz && dx && dx != dout, "sar_tattn_dx_f32: null operand, or dx is dout");
  TA_STRIDES("sar_tattn_dx_f32", d_sn, d_sc);
  TA_STRIDES("sar_tattn_dx_f32", g_sn, g_sc);
  TA_LD("sar_tattn_dx_f32", ld_dz);
  const int tps = ta_tiles_per_sample(T), ntiles = N * tps;
  int nrb = (2048 + C - 1) / C;                              // about 2048 workgroups of at least 8 tiles
  if (nrb > (ntiles + 7) / 8) nrb = (ntiles + 7) / 8;
  if (nrb > 65535) nrb = 65535;
  const int tpb = (ntiles + nrb - 1) / nrb;
  const auto k = TA_PICK(ta_dx_kernel, V, units);
  hipLaunchKernelGGL(k, dim3(C, (ntiles + tpb - 1) / tpb), dim3(TPB), 0, as_stream(s), ta_view{dout, d_sn, d_sc}, a, kernel, dz, ld_dz,
                     C, T, V, units, tps, ntiles, tpb, ta_wview{dx, g_sn, g_sc});
  SAR_LAUNCH_CHECK("sar_tattn_dx_f32");
  return 0;
}

extern "C" int sar_tattn_act_f32(float* z, int64_t ld, int rows, int64_t n, int act, sar_stream_t s) {
  SAR_REQUIRE(z && rows >= 1 && rows <= TA_UMAX && n >= 1 && n < ((int64_t)1 << 22) && ld >= n && ld < ((int64_t)1 << 31),
              "sar_tattn_act_f32: null operand, or not 1 <= rows <= %d, 1 <= n < 2^22, n <= ld < 2^31", TA_UMAX);
  SAR_REQUIRE(act == SAR_TATTN_RELU || act == SAR_TATTN_SIGMOID, "sar_tattn_act_f32: act must be SAR_TATTN_RELU or SAR_TATTN_SIGMOID (got %d)", act);
  hipLaunchKernelGGL(ta_act_kernel, dim3((unsigned)((n + TPB - 1) / TPB), rows), dim3(TPB), 0, as_stream(s), z, ld, n, act);
  SAR_LAUNCH_CHECK("sar_tattn_act_f32");
  return 0;
}

extern "C" int sar_tattn_dact_f32(const float* h, int64_t ld_h, float* dh, int64_t ld_dh, int rows, int64_t n, sar_stream_t s) {
  SAR_REQUIRE(h && dh && rows >= 1 && rows <= TA_UMAX && n >= 1 && n < ((int64_t)1 << 22) && ld_h >= n && ld_dh >= n && ld_h < ((int64_t)1 << 31) &&
                  ld_dh < ((int64_t)1 << 31),
              "sar_tattn_dact_f32: null operand, or not 1 <= rows <= %d, 1 <= n < 2^22, n <= ld < 2^31", TA_UMAX);
  hipLaunchKernelGGL(ta_dact_kernel, dim3((unsigned)((n + TPB - 1) / TPB), rows), dim3(TPB), 0, as_stream(s), h, ld_h, dh, ld_dh, n);
  SAR_LAUNCH_CHECK("sar_tattn_dact_f32");
  return 0;
}
