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
template <int WI, int WJ, int TM, int TN, int BK>
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
              if (i < a.M) cn[(int64_t)i * a.c_si + j] = acc[tm][tn][r];
            }
          }
          acc[tm][tn] = f32x16{0};
        }
    }
  }
}

template <int WI, int WJ, int TM, int TN, int BK>
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
  hipLaunchKernelGGL((gs_kernel<WI, WJ, TM, TN, BK>), dim3((unsigned)grid), dim3(TPB), 0, as_stream(s), a);
  SAR_LAUNCH_CHECK(who);
  return 0;
}

int gs_launch(const gs_args& a, int batch, const char* who, sar_stream_t s) {
  if (a.N <= 32) return gs_launch_as<4, 1, 1, 1, 32>(a, batch, who, s);
  if (a.N <= 64) return gs_launch_as<2, 2, 1, 1, 32>(a, batch, who, s);
  return gs_launch_as<2, 2, 2, 2, 32>(a, batch, who, s);
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
  return gs_launch(a, N, "sar_graph_sample_fwd_f32", s);
}

extern "C" int sar_graph_sample_bwd_data_f32(const float* dout, int64_t ld_dout, const float* A, float* dy, int64_t ld_dy, int F, int V,
                                             int N, sar_stream_t s) {
  if (int rc = gs_check("sar_graph_sample_bwd_data_f32", dout, A, dy, F, V, N, ld_dout, ld_dy)) return rc;
  gs_args a{};
  a.p = dout, a.p_sn = V, a.p_si = ld_dout, a.p_sk = 1;
  a.q = A, a.q_sn = (int64_t)V * V, a.q_sk = 1, a.q_sj = V;
  a.c = dy, a.c_sn = V, a.c_si = ld_dy;
  a.M = F, a.N = V, a.K = V;
  return gs_launch(a, N, "sar_graph_sample_bwd_data_f32", s);
}

extern "C" int sar_graph_sample_dadj_f32(const float* y, int64_t ld_y, const float* dout, int64_t ld_dout, float* dA, int F, int V, int N,
                                         sar_stream_t s) {
  if (int rc = gs_check("sar_graph_sample_dadj_f32", y, dout, dA, F, V, N, ld_y, ld_dout)) return rc;
  gs_args a{};
  a.p = y, a.p_sn = V, a.p_si = 1, a.p_sk = ld_y;
  a.q = dout, a.q_sn = V, a.q_sk = ld_dout, a.q_sj = 1;
  a.c = dA, a.c_sn = (int64_t)V * V, a.c_si = V;
  a.M = V, a.N = V, a.K = F;
  return gs_launch(a, N, "sar_graph_sample_dadj_f32", s);
}
