// graph_dense_t.hip -- the adjacency contraction with a PER-FRAME dense (trainable) adjacency At[K][T][V][V]
// (the reference's models/stgcn_debug.py SGTACN: Conv2D(3F, 1x1) then einsum 'nkctv,ktvw->nctw', every block its own table):
//
//   out[m, (b,t,w)]      = sum_k sum_v y[k F + m, (b,t,v)] At[k, t, v, w]  (+ add)  (+ BatchNorm partial sums)
//   dy[k F + m, (b,t,v)] = sum_w dout[m, (b,t,w)] At[k, t, v, w]
//   dAt[k, t, v, w]      = sum_{m, b} y[k F + m, (b,t,v)] dout[m, (b,t,w)]          (NOT reduced over frames)
//
// fp32 CN layout, fp32 MFMA (v_mfma_f32_32x32x2_f32).  For a fixed frame t each of the three is one small GEMM:
//   fwd       rows (m, b) x contraction (k, v) [75] x columns w [25 of 32]
//   bwd_data  rows (m, b) x contraction w [25 of 32] x columns (k; v) [K tiles of 32]
//   dadj      rows v [25 of 32] x contraction (m, b) x columns w [25 of 32], one accumulator tile per k
// A workgroup owns GT_TT = 4 consecutive frames (one per wave) and walks samples and 32-row chunks of the channel axis.  The wave's
// table operand -- At[:, t] in MFMA fragment order -- is loaded ONCE into registers (38 VGPRs forward, K * 16 backward) and stays
// there for every chunk: the inner loops are LDS reads of the activation operand and MFMAs only.  The contraction index of the
// 32x32x2 instruction is permuted (lanes 0-31 take the first half of the contraction, lanes 32-63 the second half, the same on both
// operands), so that a lane's activation operands are CONTIGUOUS in its LDS row (ds_read_b64 / b128).  Activation rows are staged
// with plain dword loads, 4 frames x V contiguous floats per row (a frame start is 100 bytes into the row in general: no float4),
// and results leave through an LDS transpose so that a row's 4 frames are stored as one contiguous run.
// No reduction over b in fwd / bwd_data (a sample's result does not depend on the batch); dadj sums (b, m) in a fixed order inside
// a workgroup and over sample ranges through slabs reduced by sar_slab_reduce_f32: deterministic, no atomics.
#include "sar_common.h"

namespace {

constexpr int TPB = 256;
constexpr int GT_TT = 4;                      // frames per workgroup = waves per workgroup
constexpr int GT_MR = 32;                     // rows (channels) per chunk = MFMA tile height
constexpr int GT_VMAX = 32;
constexpr int GT_KMAX = 4;
constexpr int GT_HALF = 38;                   // forward contraction steps: K * V <= 2 * GT_HALF
constexpr int GT_RS = 2 * GT_HALF + 2;        // LDS row stride of the staged y rows (b64 reads of 32 rows: conflict free)
constexpr int GT_DS = 36;                     // LDS row stride of the staged dout rows (b128 reads)
constexpr int GT_OS = GT_TT * GT_VMAX + 1;    // LDS row stride of the output transpose

// rows [m0, m0 + 32) of G stacked channel groups, columns [col, col + ncol) (ncol = frames * V <= 128) -> dst[frame][row][g V + v]
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, int rs, const float* __restrict__ src, int64_t ld, int64_t col,
                                           int G, int F, int m0, int V, int ncol) {
  const int j = threadIdx.x & 127, h = threadIdx.x >> 7;
  if (j >= ncol) return;
  const int tt = j / V, v = j - tt * V;
  float* d = dst + tt * GT_MR * rs + v;
  const float* s = src + col + j;
  for (int g = 0; g < G; ++g) {
#pragma unroll 8
    for (int i = h; i < GT_MR; i += 2) {
      const int m = m0 + i;
      d[i * rs + g * V] = (m < F) ? s[(int64_t)(g * F + m) * ld] : 0.f;
    }
  }
}

// Os[row][frame V + v] -> dst rows (row0 + i), contiguous runs of ncol floats; (+ add); the stored value is written back for the statistics
__device__ __forceinline__ void store_rows(float* __restrict__ Os, float* __restrict__ dst, int64_t ld, int64_t col, int row0, int nrows,
                                           int ncol, const float* __restrict__ add, int64_t ld_add, bool keep) {
  const int j = threadIdx.x & 127, h = threadIdx.x >> 7;
  if (j >= ncol) return;
  for (int i = h; i < nrows; i += 2) {
    float val = Os[i * GT_OS + j];
    if (add) val += add[(int64_t)(row0 + i) * ld_add + col + j];
    dst[(int64_t)(row0 + i) * ld + col + j] = val;
    if (keep) Os[i * GT_OS + j] = val;
  }
}

__global__ __launch_bounds__(TPB) void gdt_fwd_kernel(const float* __restrict__ y, int64_t ld_y, const float* __restrict__ At,
                                                      float* __restrict__ out, int64_t ld_out, int K, int F, int V, int B, int T, int BG,
                                                      float* __restrict__ partials, const float* __restrict__ add, int64_t ld_add) {
  __shared__ __attribute__((aligned(16))) float Ys[GT_TT * GT_MR * GT_RS];
  __shared__ float Os[GT_MR * GT_OS];
  const int tile = blockIdx.x, t0 = tile * GT_TT, ntt = gridDim.x;
  const int nf = (t0 + GT_TT <= T) ? GT_TT : T - t0;
  const int ncol = nf * V;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hi = lane >> 5;
  const bool live = wave < nf;
  for (int i = threadIdx.x; i < GT_TT * GT_MR * GT_RS; i += TPB) Ys[i] = 0.f;      // the pad columns K V .. 2 GT_HALF stay zero
  // this wave's table operand: step s of lane (w = li, half hi) multiplies contraction index c = hi GT_HALF + s = (k, v)
  float tb[GT_HALF];
  {
    const int c0 = hi * GT_HALF;
    int k = c0 / V, v = c0 - k * V;
    const float* tp = At + (int64_t)(t0 + wave) * V * V + li;
#pragma unroll
    for (int s = 0; s < GT_HALF; ++s) {
      tb[s] = (live && k < K && li < V) ? tp[((int64_t)k * T * V + v) * V] : 0.f;
      if (++v == V) {
        v = 0;
        ++k;
      }
    }
  }
  __syncthreads();
  const int b_hi = (blockIdx.y * BG + BG < B) ? blockIdx.y * BG + BG : B;
  const int nparts = B * ntt;
  for (int b = blockIdx.y * BG; b < b_hi; ++b) {
    const int64_t col = ((int64_t)b * T + t0) * V;
    for (int m0 = 0; m0 < F; m0 += GT_MR) {
      stage_rows(Ys, GT_RS, y, ld_y, col, K, F, m0, V, ncol);
      __syncthreads();
      if (live) {
        f32x16 acc = {0};
        const float2* ap = reinterpret_cast<const float2*>(Ys + (wave * GT_MR + li) * GT_RS + hi * GT_HALF);
#pragma unroll
        for (int s2 = 0; s2 < GT_HALF / 2; ++s2) {
          const float2 a = ap[s2];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, tb[2 * s2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, tb[2 * s2 + 1], acc, 0, 0, 0);
        }
        if (li < V) {
#pragma unroll
          for (int r = 0; r < 16; ++r) Os[mfma_row(r, hi) * GT_OS + wave * V + li] = acc[r];
        }
      }
      __syncthreads();      // every wave has read Ys (the next chunk may be staged) and written Os
      const int nrows = (F - m0 < GT_MR) ? F - m0 : GT_MR;
      store_rows(Os, out, ld_out, col, m0, nrows, ncol, add, ld_add, partials != nullptr);
      if (partials) {
        __syncthreads();
        // 8 lanes per row: (sum, sum of squares) of the row's ncol stored values in a fixed order
        const int i = threadIdx.x >> 3, q = threadIdx.x & 7;
        float s1 = 0.f, s2 = 0.f;
        for (int j = q; j < ncol; j += 8) {
          const float val = Os[i * GT_OS + j];
          s1 += val;
          s2 = fmaf(val, val, s2);
        }
        s1 += __shfl_xor(s1, 1);
        s2 += __shfl_xor(s2, 1);
        s1 += __shfl_xor(s1, 2);
        s2 += __shfl_xor(s2, 2);
        s1 += __shfl_xor(s1, 4);
        s2 += __shfl_xor(s2, 4);
        if (q == 0 && i < nrows) {
          float* pp = partials + ((int64_t)(m0 + i) * nparts + (int64_t)b * ntt + tile) * 2;
          pp[0] = s1;
          pp[1] = s2;
        }
      }
      // (the next write of Os sits behind the next chunk's staging barrier)
    }
  }
}

__global__ __launch_bounds__(TPB) void gdt_bwd_kernel(const float* __restrict__ dout, int64_t ld_d, const float* __restrict__ At,
                                                      float* __restrict__ dy, int64_t ld_dy, int K, int F, int V, int B, int T, int BG) {
  __shared__ __attribute__((aligned(16))) float Ds[GT_TT * GT_MR * GT_DS];
  __shared__ float Os[GT_MR * GT_OS];
  const int t0 = blockIdx.x * GT_TT;
  const int nf = (t0 + GT_TT <= T) ? GT_TT : T - t0;
  const int ncol = nf * V;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hi = lane >> 5;
  const bool live = wave < nf;
  for (int i = threadIdx.x; i < GT_TT * GT_MR * GT_DS; i += TPB) Ds[i] = 0.f;       // the pad columns V .. 31 stay zero
  // table operand of slice k: step s of lane (v = li, half hi) multiplies w = 16 hi + s
  float tb[GT_KMAX][16];
#pragma unroll
  for (int k = 0; k < GT_KMAX; ++k) {
    const float* tp = At + (((int64_t)k * T + t0 + wave) * V + li) * V + hi * 16;
#pragma unroll
    for (int s = 0; s < 16; ++s) tb[k][s] = (live && k < K && li < V && hi * 16 + s < V) ? tp[s] : 0.f;
  }
  __syncthreads();
  const int b_hi = (blockIdx.y * BG + BG < B) ? blockIdx.y * BG + BG : B;
  for (int b = blockIdx.y * BG; b < b_hi; ++b) {
    const int64_t col = ((int64_t)b * T + t0) * V;
    for (int m0 = 0; m0 < F; m0 += GT_MR) {
      stage_rows(Ds, GT_DS, dout, ld_d, col, 1, F, m0, V, ncol);
      __syncthreads();
      float a[16];
      if (live) {
        const float4* ap = reinterpret_cast<const float4*>(Ds + (wave * GT_MR + li) * GT_DS + hi * 16);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const float4 q = ap[s4];
          a[4 * s4] = q.x, a[4 * s4 + 1] = q.y, a[4 * s4 + 2] = q.z, a[4 * s4 + 3] = q.w;
        }
      }
      const int nrows = (F - m0 < GT_MR) ? F - m0 : GT_MR;
#pragma unroll
      for (int k = 0; k < GT_KMAX; ++k) {
        if (k < K) {
          f32x16 acc = {0};
          if (live) {
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], tb[k][s], acc, 0, 0, 0);
          }
          if (k > 0) __syncthreads();      // the previous slice's rows have left Os
          if (live && li < V) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Os[mfma_row(r, hi) * GT_OS + wave * V + li] = acc[r];
          }
          __syncthreads();                 // (k = 0: every wave has also read Ds into registers: the next chunk may be staged)
          store_rows(Os, dy, ld_dy, col, k * F + m0, nrows, ncol, nullptr, 0, false);
        }
      }
    }
  }
}

// dAt of the workgroup's 4 frames over the samples [split * per, ...) and every channel -> slab[split][K][T][V][V]
__global__ __launch_bounds__(TPB) void gdt_dadj_kernel(const float* __restrict__ y, int64_t ld_y, const float* __restrict__ dout,
                                                       int64_t ld_d, int K, int F, int V, int B, int T, int per,
                                                       float* __restrict__ slab) {
  __shared__ float Ys[GT_TT * GT_MR * GT_RS];
  __shared__ float Ds[GT_TT * GT_MR * GT_DS];
  const int t0 = blockIdx.x * GT_TT, split = blockIdx.y;
  const int nf = (t0 + GT_TT <= T) ? GT_TT : T - t0;
  const int ncol = nf * V;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hi = lane >> 5;
  const bool live = wave < nf;
  const int vi = (li < V) ? li : V - 1;      // (rows / columns >= V of the tiles are computed on a valid address and dropped)
  f32x16 acc[GT_KMAX];
#pragma unroll
  for (int k = 0; k < GT_KMAX; ++k) acc[k] = f32x16{0};
  const int b_hi = (split * per + per < B) ? split * per + per : B;
  const float* yp = Ys + (wave * GT_MR + hi) * GT_RS + vi;
  const float* dp = Ds + (wave * GT_MR + hi) * GT_DS + vi;
  for (int b = split * per; b < b_hi; ++b) {
    const int64_t col = ((int64_t)b * T + t0) * V;
    for (int m0 = 0; m0 < F; m0 += GT_MR) {
      __syncthreads();                     // the previous chunk has been read
      stage_rows(Ys, GT_RS, y, ld_y, col, K, F, m0, V, ncol);
      stage_rows(Ds, GT_DS, dout, ld_d, col, 1, F, m0, V, ncol);
      __syncthreads();
      if (live) {
#pragma unroll
        for (int s = 0; s < GT_MR / 2; ++s) {          // contraction over the chunk's rows: r = 2 s + hi
          const float dv = dp[2 * s * GT_DS];
#pragma unroll
          for (int k = 0; k < GT_KMAX; ++k)
            if (k < K) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(yp[2 * s * GT_RS + k * V], dv, acc[k], 0, 0, 0);
        }
      }
    }
  }
  if (live && li < V) {
    const int64_t n = (int64_t)K * T * V * V;
#pragma unroll
    for (int k = 0; k < GT_KMAX; ++k) {
      if (k < K) {
        float* o = slab + split * n + ((int64_t)k * T + t0 + wave) * V * V + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int v = mfma_row(r, hi);
          if (v < V) o[v * V] = acc[k][r];
        }
      }
    }
  }
}

inline int gdt_tiles(int T) { return (T + GT_TT - 1) / GT_TT; }

// samples per workgroup of fwd / bwd_data: as many as leave >= 2048 workgroups (the table operand is reused over them)
inline int gdt_bgroup(int B, int T) {
  int bg = 4;
  while (bg > 1 && (int64_t)gdt_tiles(T) * ((B + bg - 1) / bg) < 2048) bg >>= 1;
  return bg;
}

// sample ranges of dadj: a function of (B, T) only
inline int gdt_dadj_per(int B, int T) {
  int nsplit = (2048 + gdt_tiles(T) - 1) / gdt_tiles(T);
  if (nsplit > B) nsplit = B;
  return (B + nsplit - 1) / nsplit;
}

}  // namespace

static int gdt_check(const char* who, const void* a, const void* b, const void* c, int K, int F, int V, int B, int T) {
  SAR_REQUIRE(a && b && c && K > 0 && F > 0 && V > 0 && B > 0 && T > 0, "%s: bad arguments", who);
  SAR_REQUIRE(K <= GT_KMAX && V <= GT_VMAX && K * V <= 2 * GT_HALF, "%s: K = %d, V = %d: built for K <= %d, V <= %d, K * V <= %d", who, K, V,
              GT_KMAX, GT_VMAX, 2 * GT_HALF);
  SAR_REQUIRE((int64_t)B * T * V < (int64_t)1 << 31 && B <= 65535, "%s: B * T * V too large", who);
  return 0;
}

extern "C" int sar_graph_dense_t_nparts(int B, int T) { return (B > 0 && T > 0) ? B * gdt_tiles(T) : SAR_E_ARG; }

extern "C" int sar_graph_dense_t_fwd_f32(const float* y, int64_t ld_y, const float* At, float* out, int64_t ld_out, int K, int F, int V,
                                         int B, int T, float* partials, const float* add, int64_t ld_add, sar_stream_t s) {
  if (int rc = gdt_check("sar_graph_dense_t_fwd", y, At, out, K, F, V, B, T)) return rc;
  const int64_t n = (int64_t)B * T * V;
  SAR_REQUIRE(ld_y >= n && ld_out >= n && (!add || ld_add >= n), "sar_graph_dense_t_fwd: leading dimension smaller than B * T * V");
  const int bg = gdt_bgroup(B, T);
  hipLaunchKernelGGL(gdt_fwd_kernel, dim3(gdt_tiles(T), (B + bg - 1) / bg), dim3(TPB), 0, as_stream(s), y, ld_y, At, out, ld_out, K, F, V,
                     B, T, bg, partials, add, ld_add);
  SAR_LAUNCH_CHECK("sar_graph_dense_t_fwd_f32");
  return 0;
}

extern "C" int sar_graph_dense_t_bwd_data_f32(const float* dout, int64_t ld_d, const float* At, float* dy, int64_t ld_dy, int K, int F,
                                              int V, int B, int T, sar_stream_t s) {
  if (int rc = gdt_check("sar_graph_dense_t_bwd_data", dout, At, dy, K, F, V, B, T)) return rc;
  const int64_t n = (int64_t)B * T * V;
  SAR_REQUIRE(ld_d >= n && ld_dy >= n, "sar_graph_dense_t_bwd_data: leading dimension smaller than B * T * V");
  const int bg = gdt_bgroup(B, T);
  hipLaunchKernelGGL(gdt_bwd_kernel, dim3(gdt_tiles(T), (B + bg - 1) / bg), dim3(TPB), 0, as_stream(s), dout, ld_d, At, dy, ld_dy, K, F, V,
                     B, T, bg);
  SAR_LAUNCH_CHECK("sar_graph_dense_t_bwd_data_f32");
  return 0;
}

extern "C" int64_t sar_graph_dense_t_dadj_slab_floats(int K, int V, int B, int T) {
  if (K <= 0 || V <= 0 || B <= 0 || T <= 0) return SAR_E_ARG;
  const int per = gdt_dadj_per(B, T);
  return (int64_t)((B + per - 1) / per) * K * T * V * V;
}

extern "C" int sar_graph_dense_t_dadj_f32(const float* y, int64_t ld_y, const float* dout, int64_t ld_d, int K, int F, int V, int B, int T,
                                          float* slab, float* dAt, sar_stream_t s) {
  if (int rc = gdt_check("sar_graph_dense_t_dadj", y, dout, slab, K, F, V, B, T)) return rc;
  const int64_t nc = (int64_t)B * T * V;
  SAR_REQUIRE(dAt && ld_y >= nc && ld_d >= nc, "sar_graph_dense_t_dadj: bad arguments");
  const int per = gdt_dadj_per(B, T), nsplit = (B + per - 1) / per;
  hipLaunchKernelGGL(gdt_dadj_kernel, dim3(gdt_tiles(T), nsplit), dim3(TPB), 0, as_stream(s), y, ld_y, dout, ld_d, K, F, V, B, T, per, slab);
  SAR_LAUNCH_CHECK("sar_graph_dense_t_dadj_f32");
  const int64_t n = (int64_t)K * T * V * V;
  return sar_slab_reduce_f32(slab, nsplit, n, n, dAt, s);
}
