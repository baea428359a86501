// graph_sample.hip -- the adjacency contraction with a PER-SAMPLE adjacency A[N][V][V] (the reference's models/gcn.py:22-36
// GraphConv: Conv1D(filters, 1) then einsum 'ncv,nvw->ncw'; the layer both projection models put behind their pooling step):
//
//   fwd       out[m, (n,w)] = sum_v y[m, (n,v)]    A[n, v, w]
//   bwd_data  dy [m, (n,v)] = sum_w dout[m, (n,w)] A[n, v, w]
//   dadj      dA [n, v, w]  = sum_m y[m, (n,v)]    dout[m, (n,w)]
//
// fp32 CN layout (column n V + v), fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 <= V <= 512, any F.  Per sample each of the three is one
// GEMM C[i][j] = sum_k P[i][k] Q[k][j] that differs only in which tensor is P / Q / C and in their strides:
//   fwd       i = m, k = v, j = w     P = y    (k contiguous)   Q = A[n]  (j contiguous)
//   bwd_data  i = m, k = w, j = v     P = dout (k contiguous)   Q = A[n]  (k contiguous: A[n] read transposed)
//   dadj      i = v, k = m, j = w     P = y    (i contiguous)   Q = dout  (j contiguous)     C = dA[n]
// so ONE kernel serves them, given the strides.  A workgroup of 4 waves owns a BM x BN tile of C of one sample and walks the
// contraction in chunks of BK = 32: the chunk of P and of Q is staged in LDS as [k][i] / [k][j] (row stride odd: with 32 k per chunk
// a half wave of the staging writes covers 32 consecutive k of one row or 32 consecutive rows of one k, 32 distinct banks either
// way, and the MFMA operand reads -- lane (i, k & 1) -- are 32 consecutive dwords per half wave), the next chunk's global loads
// are in flight while the current one is multiplied (33 KB of LDS for the largest tile, which the compiler builds with 256 VGPRs +
// 128 AGPRs and no spills: one wave per SIMD; report in profiles/layers.txt).  Rows,
// columns and contraction indices past the end are staged as ZEROS (odd V, V and F that are no multiple of 32): there is no scalar
// tail.  Three tile shapes, chosen from the column count alone: 128 x 32 (columns <= 32), 64 x 64 (<= 64), 128 x 128 (2 x 2 MFMA
// tiles per wave).  A wave whose 32 x 32 tile lies entirely outside C issues no MFMA.
// When the contraction fits one chunk (fwd / bwd_data with V <= 32) the Q tile -- A[n] -- is staged ONCE per workgroup, which walks
// several row blocks of the sample against it (all of them once the batch alone fills the chip).  For large V, A[n] (1 MB at V = 512) is tiled; the tiles of one sample are consecutive
// workgroups of ONE XCD (the linear workgroup id is remapped: ids that are congruent mod 8 share an XCD), row block fastest, so the
// re-read operand -- the A[n] column panel shared by the row blocks, the y panel shared by the column tiles -- comes from that L2.
// Every C element is one k-ordered fmaf chain of its own sample's operands: a sample's result does not depend on the batch, there
// are no atomics and no slabs, repeated launches are bitwise equal.
//
// The graph isomorphism aggregation with a per-sample adjacency (models/gcn.py:89-93 GraphIsoConv.call:
// einsum('ncv,nvw->ncw', x, A + diag(1 + epsilon))) is the SELF instantiation of the same kernel:
//   gin fwd       out[m, (n,w)] = sum_v x[m, (n,v)]    A[n, v, w] + (1 + eps) x[m, (n,w)]
//   gin bwd_data  dx [m, (n,v)] = sum_w dout[m, (n,w)] A[n, v, w] + (1 + eps) dout[m, (n,v)]
// A + diag(..) is never materialised (at V = 512 it is 1 MB per sample, and forming it reads A, writes A_ and reads A_ again):
// the epilogue adds (1 + eps[0]) P[i][j] -- the element of the P operand at the C element's own position, contraction index = column,
// read with the stores' coalescing (32 consecutive floats per row and half wave) from the panel the workgroup has just streamed --
// with one fmaf per element.  eps is read on the device.  The plain instantiations hold no trace of it (if constexpr).
//   gin eps_grad  deps[0] = sum_{m,n,v} x[m, (n,v)] dout[m, (n,v)]    one fp32 partial per workgroup, then ONE workgroup adds the
//                                                                    partials in a fixed order in fp64: no atomics
#include "sar_common.h"

namespace {

constexpr int TPB = 256;
constexpr int GS_VMAX = 512;

struct gs_args {
  const float* p;      // P[i][k] of sample n at p + n p_sn + i p_si + k p_sk
  const float* q;      // Q[k][j] at q + n q_sn + k q_sk + j q_sj
  float* c;            // C[i][j] at c + n c_sn + i c_si + j
  int64_t p_sn, p_si, p_sk, q_sn, q_sk, q_sj, c_sn, c_si;
  int M, N, K;         // rows, columns, contraction length
  int mt, nt;          // row blocks / column tiles per sample
  int mgrid;           // workgroups that share the row blocks of one column tile (each walks every mgrid-th block)
  int64_t total;       // workgroups with work = batch * nt * mgrid
  const float* eps;    // SELF only: C[i][j] += (1 + eps[0]) P[i][k = j]  (needs p_sk == 1 and K == N)
};

// one chunk of an operand: R (= BM or BN) x BK elements, element (r, kk) at base + r sr + kk sk, zero outside [0, nr) x [0, nk)
template <int R, int BK>
__device__ __forceinline__ void load_chunk(float (&reg)[R * BK / TPB], const float* __restrict__ base, int64_t sr, int64_t sk,
                                           int nr, int nk, bool k_fast) {
#pragma unroll
  for (int e = 0; e < R * BK / TPB; ++e) {
    const int idx = threadIdx.x + e * TPB;
    const int r = k_fast ? idx / BK : idx % R, kk = k_fast ? idx % BK : idx / R;
    reg[e] = (r < nr && kk < nk) ? base[r * sr + kk * sk] : 0.f;
  }
}

template <int R, int BK>
__device__ __forceinline__ void store_chunk(float* __restrict__ lds, const float (&reg)[R * BK / TPB], bool k_fast) {
#pragma unroll
  for (int e = 0; e < R * BK / TPB; ++e) {
    const int idx = threadIdx.x + e * TPB;
    const int r = k_fast ? idx / BK : idx % R, kk = k_fast ? idx % BK : idx / R;
    lds[kk * (R + 1) + r] = reg[e];
  }
}

// WI x WJ waves, TM x TN MFMA tiles per wave: BM = 32 WI TM rows, BN = 32 WJ TN columns
template <int WI, int WJ, int TM, int TN, int BK, bool SELF>
__global__ __launch_bounds__(TPB) void gs_kernel(const gs_args a) {
  static_assert(WI * WJ * 64 == TPB, "four waves");
  constexpr int BM = 32 * WI * TM, BN = 32 * WJ * TN;
  __shared__ float Ps[BK * (BM + 1)];
  __shared__ float Qs[BK * (BN + 1)];
  // XCD-aware order: the launch has 8 * per workgroups; those with equal (blockIdx.x % 8) take consecutive work items
  const int64_t per = gridDim.x / 8;
  const int64_t vid = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;
  if (vid >= a.total) return;
  const int it0 = (int)(vid % a.mgrid), jt = (int)((vid / a.mgrid) % a.nt);
  const int64_t n = vid / ((int64_t)a.mgrid * a.nt);
  const int j0 = jt * BN;
  const int nk = (a.K + BK - 1) / BK;
  const bool q_once = nk == 1;                               // the Q tile is the same for every row block of this workgroup
  const int nit = (a.mt - it0 + a.mgrid - 1) / a.mgrid;      // row blocks of this workgroup: it0, it0 + mgrid, ..
  const int steps = nit * nk;
  const bool p_kfast = a.p_sk == 1, q_kfast = a.q_sk == 1;
  const float* pn = a.p + n * a.p_sn;
  const float* qn = a.q + n * a.q_sn + (int64_t)j0 * a.q_sj;
  float* cn = a.c + n * a.c_sn;
  float self = 0.f;
  if constexpr (SELF) self = 1.f + a.eps[0];

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hi = lane >> 5;
  const int ib = (wave % WI) * TM * 32, jb = (wave / WI) * TN * 32;
  float rp[BM * BK / TPB], rq[BN * BK / TPB];
  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = f32x16{0};

  auto fetch = [&](int step) {
    const int i0 = (it0 + (step / nk) * a.mgrid) * BM, k0 = (step % nk) * BK;
    load_chunk<BM, BK>(rp, pn + (int64_t)i0 * a.p_si + (int64_t)k0 * a.p_sk, a.p_si, a.p_sk, a.M - i0, a.K - k0, p_kfast);
    if (!(q_once && step > 0)) load_chunk<BN, BK>(rq, qn + (int64_t)k0 * a.q_sk, a.q_sj, a.q_sk, a.N - j0, a.K - k0, q_kfast);
  };

  fetch(0);
  for (int step = 0; step < steps; ++step) {
    __syncthreads();                       // the previous chunk has been multiplied
    store_chunk<BM, BK>(Ps, rp, p_kfast);
    if (!(q_once && step > 0)) store_chunk<BN, BK>(Qs, rq, q_kfast);
    __syncthreads();
    if (step + 1 < steps) fetch(step + 1);
    const int i0 = (it0 + (step / nk) * a.mgrid) * BM;
    bool live[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) live[tm][tn] = i0 + ib + tm * 32 < a.M && j0 + jb + tn * 32 < a.N;   // wave uniform
#pragma unroll 4
    for (int kk = 0; kk < BK; kk += 2) {
      float pa[TM], qb[TN];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) pa[tm] = Ps[(kk + hi) * (BM + 1) + ib + tm * 32 + li];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) qb[tn] = Qs[(kk + hi) * (BN + 1) + jb + tn * 32 + li];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          if (live[tm][tn]) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[tm], qb[tn], acc[tm][tn], 0, 0, 0);
    }
    if (step % nk == nk - 1) {             // the row block is complete: 32 consecutive floats per row and half wave
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          const int j = j0 + jb + tn * 32 + li;
          if (live[tm][tn] && j < a.N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int i = i0 + ib + tm * 32 + mfma_row(r, hi);
              if (i < a.M) {
                if constexpr (SELF) cn[(int64_t)i * a.c_si + j] = fmaf(self, pn[(int64_t)i * a.p_si + j], acc[tm][tn][r]);
                else cn[(int64_t)i * a.c_si + j] = acc[tm][tn][r];
              }
            }
          }
          acc[tm][tn] = f32x16{0};
        }
    }
  }
}

template <int WI, int WJ, int TM, int TN, int BK, bool SELF>
int gs_launch_as(gs_args a, int batch, const char* who, sar_stream_t s) {
  constexpr int BM = 32 * WI * TM, BN = 32 * WJ * TN;
  a.mt = (a.M + BM - 1) / BM;
  a.nt = (a.N + BN - 1) / BN;
  // one chunk of contraction: Q is staged once per workgroup, so a workgroup takes several row blocks -- as few workgroups per
  // column tile as still give the launch 512, two per CU (a small batch with many channels must not leave the chip idle; the figure
  // comes from the CU count and has not been tuned by measurement).  The split
  // does not change any result: every C element is computed whole by one workgroup
  a.mgrid = a.mt;
  if (a.K <= BK) {
    const int64_t want = (512 + (int64_t)batch * a.nt - 1) / ((int64_t)batch * a.nt);
    a.mgrid = (int)(want < a.mt ? want : a.mt);
  }
  a.total = (int64_t)batch * a.nt * a.mgrid;
  const int64_t grid = (a.total + 7) / 8 * 8;
  SAR_REQUIRE(grid < (int64_t)1 << 31, "%s: too many tiles for one launch", who);
  hipLaunchKernelGGL((gs_kernel<WI, WJ, TM, TN, BK, SELF>), dim3((unsigned)grid), dim3(TPB), 0, as_stream(s), a);
  SAR_LAUNCH_CHECK(who);
  return 0;
}

template <bool SELF>
int gs_launch(const gs_args& a, int batch, const char* who, sar_stream_t s) {
  if (a.N <= 32) return gs_launch_as<4, 1, 1, 1, 32, SELF>(a, batch, who, s);
  if (a.N <= 64) return gs_launch_as<2, 2, 1, 1, 32, SELF>(a, batch, who, s);
  return gs_launch_as<2, 2, 2, 2, 32, SELF>(a, batch, who, s);
}

// every limit, before any launch
int gs_check(const char* who, const void* x, const void* y, const void* z, int F, int V, int N, int64_t ld_a, int64_t ld_b) {
  SAR_REQUIRE(x && y && z && F > 0 && V > 0 && N > 0, "%s: bad arguments", who);
  if (V > GS_VMAX) {
    sar_set_error("%s: V = %d: built for V <= %d", who, V, GS_VMAX);
    return SAR_E_UNSUP;
  }
  SAR_REQUIRE((int64_t)N * V < (int64_t)1 << 31, "%s: N * V too large", who);
  SAR_REQUIRE(ld_a >= (int64_t)N * V && ld_b >= (int64_t)N * V, "%s: leading dimension smaller than N * V", who);
  return 0;
}

}  // namespace

extern "C" int sar_graph_sample_fwd_f32(const float* y, int64_t ld_y, const float* A, float* out, int64_t ld_out, int F, int V, int N,
                                        sar_stream_t s) {
  if (int rc = gs_check("sar_graph_sample_fwd_f32", y, A, out, F, V, N, ld_y, ld_out)) return rc;
  gs_args a{};
  a.p = y, a.p_sn = V, a.p_si = ld_y, a.p_sk = 1;
  a.q = A, a.q_sn = (int64_t)V * V, a.q_sk = V, a.q_sj = 1;
  a.c = out, a.c_sn = V, a.c_si = ld_out;
  a.M = F, a.N = V, a.K = V;
  return gs_launch<false>(a, N, "sar_graph_sample_fwd_f32", s);
}

extern "C" int sar_graph_sample_bwd_data_f32(const float* dout, int64_t ld_dout, const float* A, float* dy, int64_t ld_dy, int F, int V,
                                             int N, sar_stream_t s) {
  if (int rc = gs_check("sar_graph_sample_bwd_data_f32", dout, A, dy, F, V, N, ld_dout, ld_dy)) return rc;
  gs_args a{};
  a.p = dout, a.p_sn = V, a.p_si = ld_dout, a.p_sk = 1;
  a.q = A, a.q_sn = (int64_t)V * V, a.q_sk = 1, a.q_sj = V;
  a.c = dy, a.c_sn = V, a.c_si = ld_dy;
  a.M = F, a.N = V, a.K = V;
  return gs_launch<false>(a, N, "sar_graph_sample_bwd_data_f32", s);
}

extern "C" int sar_graph_sample_dadj_f32(const float* y, int64_t ld_y, const float* dout, int64_t ld_dout, float* dA, int F, int V, int N,
                                         sar_stream_t s) {
  if (int rc = gs_check("sar_graph_sample_dadj_f32", y, dout, dA, F, V, N, ld_y, ld_dout)) return rc;
  gs_args a{};
  a.p = y, a.p_sn = V, a.p_si = 1, a.p_sk = ld_y;
  a.q = dout, a.q_sn = V, a.q_sk = ld_dout, a.q_sj = 1;
  a.c = dA, a.c_sn = (int64_t)V * V, a.c_si = V;
  a.M = V, a.N = V, a.K = F;
  return gs_launch<false>(a, N, "sar_graph_sample_dadj_f32", s);
}

// ---- the graph isomorphism aggregation: the same contraction plus (1 + eps) times the operand itself
extern "C" int sar_gin_sample_fwd_f32(const float* x, int64_t ld_x, const float* A, const float* eps, float* out, int64_t ld_out, int F,
                                      int V, int N, sar_stream_t s) {
  if (int rc = gs_check("sar_gin_sample_fwd_f32", x, A, out, F, V, N, ld_x, ld_out)) return rc;
  SAR_REQUIRE(eps, "sar_gin_sample_fwd_f32: eps is NULL");
  gs_args a{};
  a.p = x, a.p_sn = V, a.p_si = ld_x, a.p_sk = 1;
  a.q = A, a.q_sn = (int64_t)V * V, a.q_sk = V, a.q_sj = 1;
  a.c = out, a.c_sn = V, a.c_si = ld_out;
  a.M = F, a.N = V, a.K = V, a.eps = eps;
  return gs_launch<true>(a, N, "sar_gin_sample_fwd_f32", s);
}

extern "C" int sar_gin_sample_bwd_data_f32(const float* dout, int64_t ld_dout, const float* A, const float* eps, float* dx, int64_t ld_dx,
                                           int F, int V, int N, sar_stream_t s) {
  if (int rc = gs_check("sar_gin_sample_bwd_data_f32", dout, A, dx, F, V, N, ld_dout, ld_dx)) return rc;
  SAR_REQUIRE(eps, "sar_gin_sample_bwd_data_f32: eps is NULL");
  gs_args a{};
  a.p = dout, a.p_sn = V, a.p_si = ld_dout, a.p_sk = 1;
  a.q = A, a.q_sn = (int64_t)V * V, a.q_sk = 1, a.q_sj = V;
  a.c = dx, a.c_sn = V, a.c_si = ld_dx;
  a.M = F, a.N = V, a.K = V, a.eps = eps;
  return gs_launch<true>(a, N, "sar_gin_sample_bwd_data_f32", s);
}

// ---- d epsilon = <x, dout> over the F x (N V) live elements.  HBM-bound: both operands are read once, 16 B per lane
namespace {

constexpr int EG_COLS = TPB * 16;       // columns of one row per work item: four float4 of each operand per lane
constexpr int EG_MAX_WG = 8192;         // workgroups (= partials) of a launch; a workgroup walks every EG_MAX_WG-th item

inline int64_t eg_chunks(int64_t n) { return (n + EG_COLS - 1) / EG_COLS; }
inline int64_t eg_workgroups(int F, int64_t n) {
  const int64_t items = (int64_t)F * eg_chunks(n);
  return items < EG_MAX_WG ? items : EG_MAX_WG;
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void eg_partial_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ d,
                                                         int64_t ld_d, int64_t n, int64_t chunks, int64_t items,
                                                         float* __restrict__ partials) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t row = it / chunks, c0 = (it % chunks) * EG_COLS;
    const float* xr = x + row * ld_x;
    const float* dr = d + row * ld_d;
    if constexpr (VEC) {
      float4 a[4], b[4];
      bool full[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t i = c0 + ((int64_t)q * TPB + threadIdx.x) * 4;
        full[q] = i + 4 <= n;
        a[q] = b[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (full[q]) {
          a[q] = *reinterpret_cast<const float4*>(xr + i);
          b[q] = *reinterpret_cast<const float4*>(dr + i);
        } else {                                              // the last, partial group of a row with n % 4 != 0
          float ta[4] = {0.f, 0.f, 0.f, 0.f}, tb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < n) ta[j] = xr[i + j], tb[j] = dr[i + j];
          a[q] = make_float4(ta[0], ta[1], ta[2], ta[3]);
          b[q] = make_float4(tb[0], tb[1], tb[2], tb[3]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[0] = fmaf(a[q].x, b[q].x, acc[0]);
        acc[1] = fmaf(a[q].y, b[q].y, acc[1]);
        acc[2] = fmaf(a[q].z, b[q].z, acc[2]);
        acc[3] = fmaf(a[q].w, b[q].w, acc[3]);
      }
    } else {
#pragma unroll 4
      for (int q = 0; q < 16; ++q) {
        const int64_t i = c0 + (int64_t)q * TPB + threadIdx.x;
        if (i < n) acc[q & 3] = fmaf(xr[i], dr[i], acc[q & 3]);
      }
    }
  }
  float v = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: the partials in a fixed order, fp64 (as bn_finalize_kernel reduces)
__global__ __launch_bounds__(TPB) void eg_final_kernel(const float* __restrict__ partials, int nparts, float* __restrict__ deps) {
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += TPB) a += (double)partials[i];
  a = wave_sum_d(a);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) deps[0] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

}  // namespace

extern "C" int64_t sar_gin_sample_eps_grad_scratch_floats(int F, int V, int N) {
  if (F <= 0 || V <= 0 || N <= 0) return SAR_E_ARG;
  return eg_workgroups(F, (int64_t)N * V);
}

extern "C" int sar_gin_sample_eps_grad_f32(const float* x, int64_t ld_x, const float* dout, int64_t ld_dout, int F, int V, int N,
                                           float* scratch, float* deps, sar_stream_t s) {
  if (int rc = gs_check("sar_gin_sample_eps_grad_f32", x, dout, deps, F, V, N, ld_x, ld_dout)) return rc;
  SAR_REQUIRE(scratch, "sar_gin_sample_eps_grad_f32: scratch is NULL");
  const int64_t n = (int64_t)N * V, chunks = eg_chunks(n), items = (int64_t)F * chunks;
  const int wgs = (int)eg_workgroups(F, n);
  const bool vec = !(ld_x & 3) && !(ld_dout & 3) && !((uintptr_t)x & 15) && !((uintptr_t)dout & 15);
  if (vec)
    hipLaunchKernelGGL(eg_partial_kernel<true>, dim3(wgs), dim3(TPB), 0, as_stream(s), x, ld_x, dout, ld_dout, n, chunks, items,
                       scratch);
  else
    hipLaunchKernelGGL(eg_partial_kernel<false>, dim3(wgs), dim3(TPB), 0, as_stream(s), x, ld_x, dout, ld_dout, n, chunks, items,
                       scratch);
  SAR_LAUNCH_CHECK("sar_gin_sample_eps_grad_f32");
  hipLaunchKernelGGL(eg_final_kernel, dim3(1), dim3(TPB), 0, as_stream(s), scratch, wgs, deps);
  SAR_LAUNCH_CHECK("sar_gin_sample_eps_grad_f32");
  return 0;
}
