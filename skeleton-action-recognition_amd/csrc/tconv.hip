// tconv.hip -- TemporalConv: a convolution along T with a run-time kernel size k, dilation d and stride s, fp32, forward and backward.
// x (N, C, T, V), out / dout (N, M, T_out, V), W the Keras kernel (k, 1, C, M) as it lies:
//
//   out[n,m,to,v] = bias[m] + sum_{j<k} sum_{c<C} W[j][c][m] x[n, c, to s + j d - pad, v]          (x is exactly 0 outside [0, T))
//   dx [n,c,u,v]  = sum_j sum_m W[j][c][m] dout[n, m, (u + pad - j d) / s, v]                        (exact quotients in [0, T_out) only)
//   dW [j][c][m]  = sum_{n,to,v} x[n, c, to s + j d - pad, v] dout[n,m,to,v]        dbias[m] = sum_{n,to,v} dout[n,m,to,v]
//
// Addressing: element (n, c, t, v) of x / out / dout / dx is at n s_n + c s_c + t V + v (csrc/gpool.hip, csrc/tattn.hip): NCHW tensors and
// the engines' CN matrices [C][ld] are the same kernels and nothing is converted.  All three products run on v_mfma_f32_32x32x2_f32
// (exact fp32 products, fp32 accumulation); k, d, s and pad are run-time arguments of ONE kernel per product.
//
//   prod    forward and data gradient are the same kernel: D[r][col] = sum_j sum_kk Wimg[j][kk][r] src[kk][col shifted by tap j].
//           Forward: r = m, kk = c, Wimg = W.  Data gradient: r = c, kk = m, Wimg = the (k, M, C) image of W (one transpose launch of
//           the caller, as conv1x1_dgrad makes it), and the tap walks the other way.  grid (column groups x parity classes, row
//           groups, N): a tile never leaves its sample, so no shift can carry a column into the neighbouring sample.  A wave owns
//           32 MB rows x 64 columns (MB = 1 where there are at most 32 rows, else 2) and reads both operands straight from global
//           memory into the MFMA operand registers (csrc/adjattn.hip's similarity): a shifted tap is the same row at a column offset,
//           there is no halo and no LDS.  Per tile the lane's column is divided into (frame, joint) once; per tile and tap the
//           frame-range test is one compare whose wave-wide ballot skips a tap that reads only padding and picks the unpredicated
//           loop where every lane is live; the contraction loop then holds operand loads and MFMAs only.  With stride 2 the data
//           gradient's columns are split by the parity of the frame u: (u + pad - j d) is even for the same taps in a whole tile, the
//           others are not issued.
//   wgrad   grid (32-channel blocks, 64-filter blocks, slabs).  The contraction index is the column (n, to, v), walked in tiles of 64
//           columns of ONE sample.  dout's tile [64 m][64 columns] is staged once per tile; wave w owns taps w, w + 4, w + 8 and
//           stages ITS tap's shifted x tile [32 c][64 columns] (coalesced along the columns, zeros outside [0, T)) into its own LDS
//           image (stage per tap: (k - 1) d reaches 64 frames, a halo tile is no option).  Row stride 66: the transposing operand
//           reads are conflict-free.  The tiles are cut into sar_tconv_wgrad_slabs(N, C, M, T_out, V) slabs -- the shape alone --,
//           every slab writes its own [k C M + M] partial (every element) and sar_slab_reduce_f32 adds them in slab order.  dbias
//           is summed per filter in column order by the workgroups of channel block 0.
// No atomics; every output element is one accumulation chain over (tap, contraction index) in a fixed order that depends on the
// shape only: bitwise deterministic, and a sample's out / dx do not depend on the rest of the batch.
#include <type_traits>

#include "sar_common.h"

namespace {

constexpr int TPB = 256;
constexpr int TC_KMAX = SAR_TCONV_KMAX, TC_DMAX = SAR_TCONV_DMAX, TC_CMAX = SAR_TCONV_CMAX, TC_VMAX = SAR_TCONV_VMAX;
constexpr int PC = 64;               // columns of a wave's tile of the product (two MFMA column blocks)
constexpr int PU = 4;                // contraction steps of the product whose operands are in flight at once
constexpr int WT = 64;               // columns of a wgrad tile
constexpr int WS = WT + 2;           // LDS row stride of its stages
constexpr int WQ = 3;                // taps per wave: w, w + 4, w + 8
constexpr int WG_TARGET = 512;       // workgroups a weight gradient aims at ..
constexpr int WG_SLAB_MAX = 256;     // .. in at most this many slabs of at least 4 tiles

struct tc_view {
  const float* p;
  int64_t sn, sc;
};
struct tc_wview {
  float* p;
  int64_t sn, sc;
};
struct tc_prod {
  int R, K;                          // output rows, contraction length
  int Tsrc, Tdst, V;                 // frames of the source and of the destination
  int k, d, s, pad;
  int dgrad;
  int ngroups;                       // workgroups along the columns of one parity class
};

// grid (parity classes * ngroups, ceil(R / 32 MB), N)
template <int MB>
__global__ __launch_bounds__(TPB) void tc_prod_kernel(const tc_view src, const float* __restrict__ W, const float* __restrict__ bias,
                                                      const tc_wview dst, const tc_prod g) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lo = lane & 31, hi = lane >> 5;
  const int n = blockIdx.z, r0 = blockIdx.y * (32 * MB);
  // column map: column -> (frame index fi, joint v); destination frame fi * ostep + par, source frame fi * a + the tap's offset
  int par = 0, grp = blockIdx.x, ostep = 1, a = g.s;
  if (g.dgrad) {
    ostep = g.s, a = 1;
    par = grp / g.ngroups;
    grp -= par * g.ngroups;
  }
  const int nf = (g.Tdst - par + ostep - 1) / ostep, ncols = nf * g.V;
  const int c0 = (grp * 4 + w) * PC;
  if (c0 >= ncols) return;           // (no barrier in this kernel)
  bool live[2];
  int fr[2], so[2], dso[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int col = c0 + nb * 32 + lo, fi = col / g.V, v = col - fi * g.V;
    live[nb] = col < ncols;
    fr[nb] = fi * a;
    so[nb] = fi * a * g.V + v;
    dso[nb] = (fi * ostep + par) * g.V + v;
  }
  int rof[MB];                       // a row past R reads row R - 1: it only reaches accumulator rows that are never stored
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) rof[mb] = r0 + mb * 32 + lo < g.R ? r0 + mb * 32 + lo : g.R - 1;
  f32x16 acc[MB][2];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc[mb][nb][reg] = 0.f;
  const float* sbase = src.p + n * src.sn + hi * src.sc;
  const int kfull = g.K & ~(2 * PU - 1);
  for (int j = 0; j < g.k; ++j) {
    int toff;                                                 // (wave-uniform)
    if (g.dgrad) {
      const int q = par + g.pad - j * g.d;
      if (g.s == 2 && (q & 1)) continue;                      // this parity class meets no output frame through tap j
      toff = g.s == 2 ? q >> 1 : q;
    } else {
      toff = j * g.d - g.pad;
    }
    bool ok[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) ok[nb] = live[nb] && (unsigned)(fr[nb] + toff) < (unsigned)g.Tsrc;
    if (__ballot(ok[0] || ok[1]) == 0) continue;              // the tap reads only padding in this tile
    const bool all = __ballot(ok[0] && ok[1]) == ~0ull;
    const float* wp = W + ((int64_t)j * g.K + hi) * g.R;               // A: Wimg[j][kk + hi][r0 + 32 mb + lo]
    const float* xp[2];                                                // B: src[kk + hi][the tap's column of column nb 32 + lo]
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) xp[nb] = sbase + (so[nb] + toff * g.V);
    auto chunk = [&](auto pred_c, int kk0) {
      constexpr bool PRED = decltype(pred_c)::value;
      float av[PU][MB], bv[PU][2];
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const bool kin = !PRED || kk0 + 2 * u + hi < g.K;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) av[u][mb] = kin ? wp[(2 * u) * g.R + rof[mb]] : 0.f;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) bv[u][nb] = (!PRED || (kin && ok[nb])) ? xp[nb][(2 * u) * src.sc] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < PU; ++u)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][mb], bv[u][nb], acc[mb][nb], 0, 0, 0);
      wp += (int64_t)(2 * PU) * g.R;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) xp[nb] += (2 * PU) * src.sc;
    };
    if (all) {
      for (int kk0 = 0; kk0 < kfull; kk0 += 2 * PU) chunk(std::false_type{}, kk0);
    } else {
      for (int kk0 = 0; kk0 < kfull; kk0 += 2 * PU) chunk(std::true_type{}, kk0);
    }
    if (kfull < g.K) chunk(std::true_type{}, kfull);
  }
  float* o = dst.p + n * dst.sn;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = r0 + mb * 32 + mfma_row(reg, hi);
      if (r >= g.R) continue;
      const float b = bias ? bias[r] : 0.f;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        if (live[nb]) o[r * dst.sc + dso[nb]] = acc[mb][nb][reg] + b;
    }
}

// grid (ceil(C / 32), ceil(M / 32 MB), slabs); tile ti = (sample ti / tps, columns 64 (ti % tps) ..)
template <int MB>
__global__ __launch_bounds__(TPB) void tc_wgrad_kernel(const tc_view x, const tc_view dy, int C, int M, int T, int Tout, int V, int k, int d,
                                                       int s, int pad, int tps, int ntiles, int tpsl, float* __restrict__ slab,
                                                       int64_t slab_stride) {
  __shared__ float xs[4][32 * WS];             // per wave: its tap's shifted tile [channel][column]
  __shared__ float ds[32 * MB * WS];           // [filter][column]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lo = lane & 31, hi = lane >> 5;
  const int c0 = blockIdx.x * 32, m0 = blockIdx.y * (32 * MB);
  const int tile0 = blockIdx.z * tpsl, tile1 = tile0 + tpsl < ntiles ? tile0 + tpsl : ntiles;
  const int ncols = Tout * V, nq = (k + 3) >> 2;
  const bool sums = blockIdx.x == 0 && tid < 32 * MB;
  // a channel past C / a filter past M reads the last one: it only reaches accumulator rows / columns that are never stored
  const int mw = m0 + w < M ? m0 + w : M - 1;  // this lane's first filter of the dout stage
  int cl = C - 1 - c0, ml = M - 1 - mw;
  asm volatile("" : "+v"(cl), "+v"(ml));       // kept per lane: 32 + 16 uniform row offsets would live in (and spill from) scalar registers
  f32x16 acc[WQ][MB];
#pragma unroll
  for (int q = 0; q < WQ; ++q)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc[q][mb][reg] = 0.f;
  float bsum = 0.f;
  const float* xa = xs[w] + lo * WS + hi;      // A: x tile [c0 + lo][column 2 st + hi]
  const float* db = ds + lo * WS + hi;         // B: dout tile [m0 + 32 mb + lo][column 2 st + hi]
  for (int ti = tile0; ti < tile1; ++ti) {
    const int n = ti / tps, col = (ti - n * tps) * WT + lane, to = col / V, v = col - to * V;
    const bool live = col < ncols;
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      if (q >= nq) break;                      // (the workgroup's trip count: every wave meets every barrier)
      const int tap = w + 4 * q, ts = to * s + tap * d - pad;
      const bool ok = tap < k && live && (unsigned)ts < (unsigned)T;
      const bool any = __ballot(ok) != 0;      // (wave-uniform) the tap reads only padding in this tile: nothing to add
      __syncthreads();                         // the previous round's operands have been read
      if (q == 0) {
        const float* dp = dy.p + n * dy.sn + mw * dy.sc + col;
        float dr[8 * MB];
#pragma unroll
        for (int i = 0; i < 8 * MB; ++i) dr[i] = 0.f;
        if (live) {
#pragma unroll
          for (int i = 0; i < 8 * MB; ++i) {
            dr[i] = *dp;
            if (4 * i + 4 <= ml) dp += 4 * dy.sc;
          }
        }
#pragma unroll
        for (int i = 0; i < 8 * MB; ++i) ds[(w + 4 * i) * WS + lane] = dr[i];
      }
      if (any) {
        const float* xp = x.p + n * x.sn + c0 * x.sc + (ts * V + v);
        float xr[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) xr[r] = 0.f;
        if (ok) {
#pragma unroll
          for (int r = 0; r < 32; ++r) {
            xr[r] = *xp;
            if (r < cl) xp += x.sc;
          }
        }
#pragma unroll
        for (int r = 0; r < 32; ++r) xs[w][r * WS + lane] = xr[r];
      }
      __syncthreads();
      if (any) {
#pragma unroll 8
        for (int st = 0; st < WT; st += 2) {
          const float av = xa[st];
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) acc[q][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, db[mb * 32 * WS + st], acc[q][mb], 0, 0, 0);
        }
      }
      if (q == 0 && sums)
        for (int cc = 0; cc < WT; ++cc) bsum += ds[tid * WS + cc];
    }
  }
  float* o = slab + blockIdx.z * slab_stride;
  if (sums && m0 + tid < M) o[(int64_t)k * C * M + m0 + tid] = bsum;
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int tap = w + 4 * q;
    if (tap >= k) continue;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = m0 + mb * 32 + lo;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int c = c0 + mfma_row(reg, hi);
        if (c < C && m < M) o[((int64_t)tap * C + c) * M + m] = acc[q][mb][reg];
      }
    }
  }
}

inline int tc_wgrad_mb(int M) { return M <= 32 ? 1 : 2; }
inline int tc_tiles_per_sample(int Tout, int V) { return (Tout * V + WT - 1) / WT; }

// slabs of the weight gradient: about WG_TARGET workgroups, at least 4 tiles a slab, at most WG_SLAB_MAX slabs -- the shape alone
inline int tc_slabs(int N, int C, int M, int Tout, int V) {
  const int64_t ntiles = (int64_t)N * tc_tiles_per_sample(Tout, V);
  const int wgs = ((C + 31) / 32) * ((M + 32 * tc_wgrad_mb(M) - 1) / (32 * tc_wgrad_mb(M)));
  int64_t s = (WG_TARGET + wgs - 1) / wgs;
  if (s > (ntiles + 3) / 4) s = (ntiles + 3) / 4;
  if (s > WG_SLAB_MAX) s = WG_SLAB_MAX;
  return s < 1 ? 1 : (int)s;
}

// every limit, before any launch
int tc_dims(const char* who, int N, int C, int M, int T, int Tout, int V, int k, int d, int s, int pad) {
  SAR_REQUIRE(N >= 1 && C >= 1 && M >= 1 && T >= 1 && Tout >= 1 && V >= 1 && k >= 1 && d >= 1 && s >= 1 && pad >= 0,
              "%s: need N, C, M, T, T_out, V, k, d, s >= 1 and pad >= 0 (got %d, %d, %d, %d, %d, %d; k = %d, d = %d, s = %d, pad = %d)", who, N, C, M,
              T, Tout, V, k, d, s, pad);
  if (k > TC_KMAX || d > TC_DMAX || s > 2 || pad > (k - 1) * d || C > TC_CMAX || M > TC_CMAX || V > TC_VMAX || N > 65535 ||
      (int64_t)N * C * T * V >= ((int64_t)1 << 31) || (int64_t)N * M * Tout * V >= ((int64_t)1 << 31)) {
    sar_set_error("%s: built for k <= %d, d <= %d, s in {1, 2}, pad <= (k - 1) d, C, M <= %d, V <= %d, N <= 65535 and fewer than 2^31 elements per "
                  "tensor (got N = %d, C = %d, M = %d, T = %d, T_out = %d, V = %d; k = %d, d = %d, s = %d, pad = %d)",
                  who, TC_KMAX, TC_DMAX, TC_CMAX, TC_VMAX, N, C, M, T, Tout, V, k, d, s, pad);
    return SAR_E_UNSUP;
  }
  // the last output frame's window may pass the last frame by at most pad + 1 frames (SAME puts the odd frame of padding there)
  SAR_REQUIRE((int64_t)(Tout - 1) * s + (int64_t)(k - 1) * d - pad <= (int64_t)T + pad,
              "%s: T_out = %d reads past what pad = %d allows (T = %d, k = %d, d = %d, s = %d)", who, Tout, pad, T, k, d, s);
  return 0;
}

// the runs of W floats of a strided (N, C, T, V) tensor lie inside it and do not overlap (csrc/gpool.hip, csrc/tattn.hip)
bool tc_strides_ok(int64_t sn, int64_t sc, int N, int C, int64_t W) {
  const int64_t lim = (int64_t)1 << 31;
  if (sn < 1 || sc < 1 || sn >= lim || sc >= lim) return false;
  const bool nchw = sc >= W && (C == 1 || N == 1 || sn >= (int64_t)C * sc), cn = sn >= W && (N == 1 || C == 1 || sc >= (int64_t)N * sn);
  return (nchw || cn) && (N - 1) * sn + (C - 1) * sc + W <= lim;
}

}  // namespace

#define TC_DIMS(name) \
  if (int rc__ = tc_dims(name, N, C, M, T, T_out, V, k, d, s, pad)) return rc__
#define TC_STRIDES(name, sn, sc, ch, frames)                                                                                              \
  SAR_REQUIRE(tc_strides_ok(sn, sc, N, ch, (int64_t)(frames) * V), "%s: strides (%lld, %lld) do not describe a (N, %d, %d, V) tensor", name, \
              (long long)(sn), (long long)(sc), ch, frames)

static int tc_launch_prod(const char* name, const tc_view src, const float* Wimg, const float* bias, const tc_wview dst, int N, tc_prod g,
                          sar_stream_t st) {
  const int classes = g.dgrad ? g.s : 1, nf = (g.Tdst + classes - 1) / classes;
  g.ngroups = (nf * g.V + 4 * PC - 1) / (4 * PC);
  const int mb = g.R <= 32 ? 1 : 2;
  const dim3 grid(classes * g.ngroups, (g.R + 32 * mb - 1) / (32 * mb), N);
  hipLaunchKernelGGL(mb == 1 ? tc_prod_kernel<1> : tc_prod_kernel<2>, grid, dim3(TPB), 0, as_stream(st), src, Wimg, bias, dst, g);
  SAR_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int sar_tconv_fwd_f32(const float* x, int64_t s_n, int64_t s_c, const float* kernel, const float* bias, int N, int C, int M, int T,
                                 int T_out, int V, int k, int d, int s, int pad, float* out, int64_t o_sn, int64_t o_sc, sar_stream_t st) {
  TC_DIMS("sar_tconv_fwd_f32");
  SAR_REQUIRE(x && kernel && out, "sar_tconv_fwd_f32: null operand");
  SAR_REQUIRE(out != x && out != kernel && out != bias, "sar_tconv_fwd_f32: the output is an input");
  TC_STRIDES("sar_tconv_fwd_f32", s_n, s_c, C, T);
  TC_STRIDES("sar_tconv_fwd_f32", o_sn, o_sc, M, T_out);
  return tc_launch_prod("sar_tconv_fwd_f32", tc_view{x, s_n, s_c}, kernel, bias, tc_wview{out, o_sn, o_sc}, N,
                        tc_prod{M, C, T, T_out, V, k, d, s, pad, 0, 0}, st);
}

extern "C" int sar_tconv_bwd_data_f32(const float* dout, int64_t d_sn, int64_t d_sc, const float* kernel_t, int N, int C, int M, int T, int T_out,
                                      int V, int k, int d, int s, int pad, float* dx, int64_t g_sn, int64_t g_sc, sar_stream_t st) {
  TC_DIMS("sar_tconv_bwd_data_f32");
  SAR_REQUIRE(dout && kernel_t && dx, "sar_tconv_bwd_data_f32: null operand");
  SAR_REQUIRE(dx != dout && dx != kernel_t, "sar_tconv_bwd_data_f32: the output is an input");
  TC_STRIDES("sar_tconv_bwd_data_f32", d_sn, d_sc, M, T_out);
  TC_STRIDES("sar_tconv_bwd_data_f32", g_sn, g_sc, C, T);
  return tc_launch_prod("sar_tconv_bwd_data_f32", tc_view{dout, d_sn, d_sc}, kernel_t, nullptr, tc_wview{dx, g_sn, g_sc}, N,
                        tc_prod{C, M, T_out, T, V, k, d, s, pad, 1, 0}, st);
}

extern "C" int sar_tconv_wgrad_slabs(int N, int C, int M, int T_out, int V) {
  if (int rc = tc_dims("sar_tconv_wgrad_slabs", N, C, M, T_out, T_out, V, 1, 1, 1, 0)) return rc;
  return tc_slabs(N, C, M, T_out, V);
}

extern "C" int sar_tconv_wgrad_f32(const float* x, int64_t s_n, int64_t s_c, const float* dout, int64_t d_sn, int64_t d_sc, int N, int C, int M,
                                   int T, int T_out, int V, int k, int d, int s, int pad, float* slab, int nslab, sar_stream_t st) {
  TC_DIMS("sar_tconv_wgrad_f32");
  SAR_REQUIRE(x && dout && slab, "sar_tconv_wgrad_f32: null operand");
  SAR_REQUIRE(slab != x && slab != dout, "sar_tconv_wgrad_f32: the output is an input");
  SAR_REQUIRE(nslab == tc_slabs(N, C, M, T_out, V), "sar_tconv_wgrad_f32: nslab must be sar_tconv_wgrad_slabs(N, C, M, T_out, V) = %d (got %d)",
              tc_slabs(N, C, M, T_out, V), nslab);
  TC_STRIDES("sar_tconv_wgrad_f32", s_n, s_c, C, T);
  TC_STRIDES("sar_tconv_wgrad_f32", d_sn, d_sc, M, T_out);
  const int tps = tc_tiles_per_sample(T_out, V), ntiles = N * tps, tpsl = (ntiles + nslab - 1) / nslab, mb = tc_wgrad_mb(M);
  const dim3 grid((C + 31) / 32, (M + 32 * mb - 1) / (32 * mb), nslab);
  hipLaunchKernelGGL(mb == 1 ? tc_wgrad_kernel<1> : tc_wgrad_kernel<2>, grid, dim3(TPB), 0, as_stream(st), tc_view{x, s_n, s_c},
                     tc_view{dout, d_sn, d_sc}, C, M, T, T_out, V, k, d, s, pad, tps, ntiles, tpsl, slab, (int64_t)k * C * M + M);
  SAR_LAUNCH_CHECK("sar_tconv_wgrad_f32");
  return 0;
}
