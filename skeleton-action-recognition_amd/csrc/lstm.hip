// lstm.hip -- the kernels behind models/lstm_sampler.py (the reference's models/lstm_sampler.py:1-27, TemporalSampler): a Keras LSTM
// layer's recurrence as ONE launch over all T steps (forward and backward through time), the fixed-order top-k of the frame scores,
// the frame gather with its gradients, and the layout change between (N, C, T, V) and the stack's CN matrices.
//
// Layout of the stack: fp32 CN matrices [rows][ld] with TIME-MAJOR columns t*N + n.  The 16 sequences a workgroup owns are then
// contiguous at every step, and h_{t-1} as a matrix is h shifted by N columns (the recurrent weight gradient takes views).
//
// The recurrence (Keras LSTM, gate order i, f, c, o along the 4u axis; zin = kernel^T x + bias is formed by the caller's 1x1 product):
//   z_t = zin_t + U^T h_{t-1};  i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_c);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
// lstm_fwd_kernel<UB>: one workgroup per tile of LSTM_NT = 16 sequences, UB = ceil(u / 16) waves.  Wave w owns the hidden units
// 16 w .. 16 w + 15: four 16x16 MFMA tiles (one per gate, rows = its units, columns = the sequences), so a lane holds the four gates
// of the same (unit, sequence) pairs -- unit 16 w + 4 (lane >> 4) + r, r = 0..3, sequence lane & 15 -- and the gate functions need no
// exchange.  U stays in registers for the whole launch as the A operands (16 UB floats per lane: U^T[gate row][k] with the hidden
// width padded to KP = 16 UB by ZERO operands, never by out-of-range reads); c stays in registers; h_{t-1} is exchanged through a
// double-buffered LDS tile [KP][16] (the B operand of k-step kk is the contiguous 64 floats 64 kk .. 64 kk + 63: no bank
// conflicts), ONE barrier per step.  The accumulators start from zin (prefetched one step ahead), so z = zin + U^T h is the MFMA
// chain itself: 4 UB dependent v_mfma_f32_16x16x4_f32 per gate, the four gates' chains independent (they hide the 40-cycle
// dependent latency).  An MFMA column depends on its own B column only: a sequence's result does not depend on which other
// sequences share its tile or launch, bit for bit.  Saved for backward: the post-activation gates [4u][T N] and c [u][T N]
// (tanh(c) is recomputed).
// lstm_bwd_kernel<UB>: the same residency scheme walking t = T-1 .. 0: dz_t from dh_out_t + dh carried, the saved gates, c_t and
// c_{t-1}; dz_t goes to global memory and to a double-buffered LDS tile [4][KP][16]; dh_{t-1} += U dz_t is four independent chains
// of 4 UB MFMAs (one per gate's k range) added in a fixed order; dc is carried in registers.  No atomics anywhere in this file:
// repeated launches are bitwise equal.
#include "sar_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define LSTM_NT 16          // sequences per workgroup: one MFMA column tile
#define LSTM_MAX_U 128
#define TOPK_MAX_T 2048
#define TOPK_THREADS 1024
#define PACK_NT 64          // pack / unpack tile: 64 sequences x 32 joints
#define PACK_VT 32

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <int UB>
__global__ __launch_bounds__(64 * UB) void lstm_fwd_kernel(const float* __restrict__ zin, int64_t ld_z, const float* __restrict__ U,
                                                           float* __restrict__ h, int64_t ld_h, float* __restrict__ gates, int64_t ld_g,
                                                           float* __restrict__ cs, int64_t ld_c, int u, int N, int T) {
  constexpr int KP = 16 * UB, KS = 4 * UB;
  __shared__ float hs[2][KP * LSTM_NT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int n = blockIdx.x * LSTM_NT + l15, j0 = wave * 16;
  const bool seq_ok = n < N;
  // A operands: a[q][kk] = U^T[q u + j0 + l15][4 kk + l4] = U[4 kk + l4][q u + j0 + l15]; zero outside u x u
  float a[4][KS];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int k = 4 * kk + l4, col = j0 + l15;
      a[q][kk] = (k < u && col < u) ? U[(int64_t)k * 4 * u + q * u + col] : 0.f;
    }
  for (int i = tid; i < KP * LSTM_NT; i += 64 * UB) hs[0][i] = 0.f;      // h_{-1} = 0
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  const int unit0 = j0 + 4 * l4;                                         // this lane's units unit0 + r
  // Pointers advance by N per step.  Loads are UNCONDITIONAL from clamped addresses (row min(unit, u - 1), sequence min(n, N - 1)):
  // a dead lane (padded unit or sequence) computes on a copy of live data, its h is forced to zero below (a padded unit) or is one
  // more column of the tile (a padded sequence; MFMA columns are independent), and nothing of it is stored.  No select sits
  // between a load and its use: the compiler turns one into a branch with a full wait behind every load (7.5 us per step, measured).
  const int nc = min(n, N - 1);
  const float* zl = zin + nc;
  int64_t zrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) zrow[r] = (int64_t)min(unit0 + r, u - 1) * ld_z;
  float* hl = h + ((int64_t)unit0 * ld_h + n);
  float* gl = gates + ((int64_t)unit0 * ld_g + n);
  float* cl = cs + ((int64_t)unit0 * ld_c + n);
  float zn[4][4];                                                        // zin of the coming step, [gate][r]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) zn[q][r] = zl[(int64_t)q * u * ld_z + zrow[r]];
  __syncthreads();
  for (int t = 0; t < T; ++t, zl += N, hl += N, gl += N, cl += N) {
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{zn[q][0], zn[q][1], zn[q][2], zn[q][3]};
    if (t + 1 < T) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) zn[q][r] = zl[(int64_t)q * u * ld_z + zrow[r] + N];
    }
    const float* hb = hs[t & 1];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const float b = hb[64 * kk + lane];                                // h_{t-1}[k = 4 kk + l4][sequence l15]
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][kk], b, acc[q], 0, 0, 0);
    }
    float* hw = hs[(t + 1) & 1];
    float gi[4], gf[4], gg[4], go[4], hh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gi[r] = lstm_sigmoid(acc[0][r]), gf[r] = lstm_sigmoid(acc[1][r]), gg[r] = tanhf(acc[2][r]), go[r] = lstm_sigmoid(acc[3][r]);
      c[r] = fmaf(gf[r], c[r], gi[r] * gg[r]);
      hh[r] = unit0 + r < u ? go[r] * tanhf(c[r]) : 0.f;                 // a padded unit's h stays a zero operand
      hw[(unit0 + r) * LSTM_NT + l15] = hh[r];
    }
    // The coming step's zin has had the MFMA chain and the gate functions to arrive: wait for it HERE, in front of the stores.
    // Left to the compiler the wait lands behind them, and as the stores sit under lane conditions it must be vmcnt(0): every
    // step would wait for its own stores' round trip.  (0x0F70 = s_waitcnt vmcnt(0) alone.)
    __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (unit0 + r < u && seq_ok) {
        hl[r * ld_h] = hh[r];
        if (gates != nullptr) {
          gl[(int64_t)r * ld_g] = gi[r];
          gl[(int64_t)(u + r) * ld_g] = gf[r];
          gl[(int64_t)(2 * u + r) * ld_g] = gg[r];
          gl[(int64_t)(3 * u + r) * ld_g] = go[r];
          cl[r * ld_c] = c[r];
        }
      }
    }
    __syncthreads();      // h_t is complete; every wave has read h_{t-1} (its reads precede its barrier), whose buffer step t + 1 rewrites
  }
}

template <int UB>
__global__ __launch_bounds__(64 * UB) void lstm_bwd_kernel(const float* __restrict__ dh_out, int64_t ld_dh, const float* __restrict__ gates,
                                                           int64_t ld_g, const float* __restrict__ cs, int64_t ld_c,
                                                           const float* __restrict__ U, float* __restrict__ dz, int64_t ld_dz, int u, int N,
                                                           int T) {
  constexpr int KP = 16 * UB, KS = 4 * UB;
  extern __shared__ __attribute__((aligned(16))) float lstm_smem[];      // dz_t: [2][4][KP][16]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int n = blockIdx.x * LSTM_NT + l15, j0 = wave * 16;
  const bool seq_ok = n < N;
  // A operands: a[q][kk] = U[j0 + l15][q u + 4 kk + l4]; zero outside u x u
  float a[4][KS];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int row = j0 + l15, k = 4 * kk + l4;
      a[q][kk] = (row < u && k < u) ? U[(int64_t)row * 4 * u + q * u + k] : 0.f;
    }
  const int unit0 = j0 + 4 * l4;
  float dhr[4] = {0.f, 0.f, 0.f, 0.f}, dcc[4] = {0.f, 0.f, 0.f, 0.f};    // dh and dc carried from step t + 1
  float g[4][4], ct[4], cp[4], dho[4];                                   // the coming step's operands
  // Loads are UNCONDITIONAL from clamped addresses (row min(unit, u - 1), sequence min(n, N - 1), c_{-1} read as c_0 and
  // multiplied by zero): a dead lane computes on a copy of live data, a padded unit's dz is forced to zero before it becomes an
  // MFMA operand, and nothing of a dead lane is stored.  No select sits between a load and its use (see lstm_fwd_kernel).
  const int nc = min(n, N - 1);
  const float* gl = gates + nc;
  const float* cl = cs + nc;
  const float* dl = dh_out + nc;
  float* zl = dz + ((int64_t)unit0 * ld_dz + n);
  auto load_step = [&](int t) {
    const int64_t tn = (int64_t)t * N, tp = (int64_t)max(t - 1, 0) * N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = min(unit0 + r, u - 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) g[q][r] = gl[(q * u + row) * ld_g + tn];
      ct[r] = cl[row * ld_c + tn];
      cp[r] = cl[row * ld_c + tp];
      dho[r] = dl[row * ld_dh + tn];
    }
  };
  load_step(T - 1);
  for (int t = T - 1; t >= 0; --t) {
    const int64_t tn = (int64_t)t * N;
    float* db = lstm_smem + (t & 1) * (4 * KP * LSTM_NT);
    const float first = t > 0 ? 1.f : 0.f;                               // c_{-1} = 0
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int unit = unit0 + r;
      const float gi = g[0][r], gf = g[1][r], gg = g[2][r], go = g[3][r];
      const float dh = dho[r] + dhr[r];
      const float tc = tanhf(ct[r]);
      const float dc = fmaf(dh * go, 1.f - tc * tc, dcc[r]);
      dcc[r] = dc * gf;
      const bool live = unit < u;                                        // a padded unit's dz is a zero operand
      const float dzi = live ? dc * gg * gi * (1.f - gi) : 0.f, dzf = live ? dc * (cp[r] * first) * gf * (1.f - gf) : 0.f,
                  dzg = live ? dc * gi * (1.f - gg * gg) : 0.f, dzo = live ? dh * tc * go * (1.f - go) : 0.f;
      db[(0 * KP + unit) * LSTM_NT + l15] = dzi;
      db[(1 * KP + unit) * LSTM_NT + l15] = dzf;
      db[(2 * KP + unit) * LSTM_NT + l15] = dzg;
      db[(3 * KP + unit) * LSTM_NT + l15] = dzo;
      if (seq_ok && unit < u) {
        zl[(int64_t)r * ld_dz + tn] = dzi;
        zl[(int64_t)(u + r) * ld_dz + tn] = dzf;
        zl[(int64_t)(2 * u + r) * ld_dz + tn] = dzg;
        zl[(int64_t)(3 * u + r) * ld_dz + tn] = dzo;
      }
    }
    if (t == 0) break;
    load_step(t - 1);
    __syncthreads();      // dz_t is complete; the buffer of step t + 1 was last read before this barrier, step t - 1 rewrites it
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][kk], db[q * KP * LSTM_NT + 64 * kk + lane], acc[q], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) dhr[r] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
  }
}

static int lstm_check(const char* name, int u, int N, int T) {
  SAR_REQUIRE(u >= 1 && N >= 1 && T >= 1, "%s: bad sizes u=%d N=%d T=%d", name, u, N, T);
  SAR_REQUIRE((int64_t)T * N < ((int64_t)1 << 31), "%s: T*N = %lld columns (built for fewer than 2^31)", name, (long long)T * N);
  if (u > LSTM_MAX_U) {
    sar_set_error("%s: built for u <= %d (got %d)", name, LSTM_MAX_U, u);
    return SAR_E_UNSUP;
  }
  return 0;
}

template <int UB>
static void lstm_fwd_launch(const float* zin, int64_t ld_z, const float* U, float* h, int64_t ld_h, float* gates, int64_t ld_g, float* c,
                            int64_t ld_c, int u, int N, int T, hipStream_t st) {
  lstm_fwd_kernel<UB><<<(unsigned)((N + LSTM_NT - 1) / LSTM_NT), 64 * UB, 0, st>>>(zin, ld_z, U, h, ld_h, gates, ld_g, c, ld_c, u, N, T);
}

template <int UB>
static void lstm_bwd_launch(const float* dh, int64_t ld_dh, const float* gates, int64_t ld_g, const float* c, int64_t ld_c, const float* U,
                            float* dz, int64_t ld_dz, int u, int N, int T, hipStream_t st) {
  const size_t lds = (size_t)2 * 4 * 16 * UB * LSTM_NT * sizeof(float);      // <= 64 KiB at UB = 8
  lstm_bwd_kernel<UB><<<(unsigned)((N + LSTM_NT - 1) / LSTM_NT), 64 * UB, lds, st>>>(dh, ld_dh, gates, ld_g, c, ld_c, U, dz, ld_dz, u, N, T);
}

#define LSTM_DISPATCH(fn, ...)                 \
  switch ((u + 15) / 16) {                     \
    case 1: fn<1>(__VA_ARGS__); break;         \
    case 2: fn<2>(__VA_ARGS__); break;         \
    case 3: fn<3>(__VA_ARGS__); break;         \
    case 4: fn<4>(__VA_ARGS__); break;         \
    case 5: fn<5>(__VA_ARGS__); break;         \
    case 6: fn<6>(__VA_ARGS__); break;         \
    case 7: fn<7>(__VA_ARGS__); break;         \
    default: fn<8>(__VA_ARGS__); break;        \
  }

extern "C" int sar_lstm_fwd_f32(const float* zin, int64_t ld_zin, const float* U, float* h, int64_t ld_h, float* gates, int64_t ld_gates,
                                float* c, int64_t ld_c, int u, int N, int T, sar_stream_t s) {
  SAR_REQUIRE(zin != nullptr && U != nullptr && h != nullptr, "sar_lstm_fwd_f32: null zin / U / h");
  if (int rc = lstm_check("sar_lstm_fwd_f32", u, N, T)) return rc;
  const int64_t n = (int64_t)T * N;
  SAR_REQUIRE((gates == nullptr) == (c == nullptr), "sar_lstm_fwd_f32: gates and c are saved together or not at all");
  SAR_REQUIRE(ld_zin >= n && ld_h >= n && (gates == nullptr || (ld_gates >= n && ld_c >= n)),
              "sar_lstm_fwd_f32: leading dimension smaller than T*N");
  LSTM_DISPATCH(lstm_fwd_launch, zin, ld_zin, U, h, ld_h, gates, ld_gates, c, ld_c, u, N, T, as_stream(s));
  SAR_LAUNCH_CHECK("sar_lstm_fwd_f32");
  return 0;
}

extern "C" int sar_lstm_bwd_f32(const float* dh, int64_t ld_dh, const float* gates, int64_t ld_gates, const float* c, int64_t ld_c,
                                const float* U, float* dz, int64_t ld_dz, int u, int N, int T, sar_stream_t s) {
  SAR_REQUIRE(dh != nullptr && gates != nullptr && c != nullptr && U != nullptr && dz != nullptr, "sar_lstm_bwd_f32: null operand");
  if (int rc = lstm_check("sar_lstm_bwd_f32", u, N, T)) return rc;
  const int64_t n = (int64_t)T * N;
  SAR_REQUIRE(ld_dh >= n && ld_gates >= n && ld_c >= n && ld_dz >= n, "sar_lstm_bwd_f32: leading dimension smaller than T*N");
  LSTM_DISPATCH(lstm_bwd_launch, dh, ld_dh, gates, ld_gates, c, ld_c, U, dz, ld_dz, u, N, T, as_stream(s));
  SAR_LAUNCH_CHECK("sar_lstm_bwd_f32");
  return 0;
}

// ---- top-k of a sequence's frame scores: descending by score, equal scores in ascending frame index (tf.math.top_k's tie rule).
// One workgroup per sequence: a bitonic sort in LDS of 64-bit keys (the score mapped to an unsigned integer of the same order,
// complemented | the frame index), ascending.  The integer keys are a total order whatever the scores hold, so with NaN among them
// idx is still a permutation's first k entries; -0 is keyed as +0 (they compare equal).  Padding keys are all ones: behind every frame.
__global__ __launch_bounds__(TOPK_THREADS) void topk_desc_kernel(const float* __restrict__ scores, int64_t sn, int64_t st, int T, int k,
                                                                 int P, float* __restrict__ values, int32_t* __restrict__ idx,
                                                                 int32_t* __restrict__ inv) {
  __shared__ unsigned long long key[TOPK_MAX_T];
  const int tid = threadIdx.x;
  const float* sc = scores + (int64_t)blockIdx.x * sn;
  for (int i = tid; i < P; i += TOPK_THREADS) {
    unsigned long long kv = ~0ull;
    if (i < T) {
      float x = sc[(int64_t)i * st];
      if (x == 0.f) x = 0.f;
      const uint32_t b = __float_as_uint(x), m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
      kv = ((unsigned long long)(~m) << 32) | (uint32_t)i;
    }
    key[i] = kv;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (P >> 1); i += TOPK_THREADS) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const unsigned long long x = key[lo], y = key[hi];
        if ((x > y) == ((lo & size) == 0)) key[lo] = y, key[hi] = x;
      }
      __syncthreads();
    }
  for (int j = tid; j < T; j += TOPK_THREADS) {
    const int t = (int)(uint32_t)key[j];                                  // a frame index in [0, T): the padding keys sort behind
    if (j < k) {
      idx[(int64_t)blockIdx.x * k + j] = t;
      values[(int64_t)blockIdx.x * k + j] = sc[(int64_t)t * st];
    }
    inv[(int64_t)blockIdx.x * T + t] = j < k ? j : -1;
  }
}

extern "C" int sar_topk_desc_f32(const float* scores, int64_t stride_n, int64_t stride_t, int N, int T, int k, float* values, int32_t* idx,
                                 int32_t* inv, sar_stream_t s) {
  SAR_REQUIRE(scores != nullptr && values != nullptr && idx != nullptr && inv != nullptr, "sar_topk_desc_f32: null operand");
  SAR_REQUIRE(N >= 1 && T >= 1 && stride_n >= 1 && stride_t >= 1, "sar_topk_desc_f32: bad sizes N=%d T=%d strides %lld %lld", N, T,
              (long long)stride_n, (long long)stride_t);
  SAR_REQUIRE(k >= 1 && k <= T, "sar_topk_desc_f32: need 1 <= k <= T (got k=%d, T=%d)", k, T);
  if (T > TOPK_MAX_T) {
    sar_set_error("sar_topk_desc_f32: built for T <= %d (got %d)", TOPK_MAX_T, T);
    return SAR_E_UNSUP;
  }
  int P = 1;
  while (P < T) P <<= 1;
  topk_desc_kernel<<<(unsigned)N, TOPK_THREADS, 0, as_stream(s)>>>(scores, stride_n, stride_t, T, k, P, values, idx, inv);
  SAR_LAUNCH_CHECK("sar_topk_desc_f32");
  return 0;
}

// ---- out[n, c, j, v] = x[n, c, idx[n, j], v] * values[n, j]: one multiply per element, both tensors NCHW
__global__ __launch_bounds__(256) void frame_gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ values, float* __restrict__ out, int C, int T, int V,
                                                           int k, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int v = (int)(e % V);
  const int64_t r = e / V;
  const int j = (int)(r % k);
  const int64_t nc = r / k, n = nc / C;
  const int t = min(max(idx[n * k + j], 0), T - 1);
  out[e] = x[(nc * T + t) * V + v] * values[n * k + j];
}

extern "C" int sar_frame_gather_f32(const float* x, const int32_t* idx, const float* values, float* out, int N, int C, int T, int V, int k,
                                    sar_stream_t s) {
  SAR_REQUIRE(x != nullptr && idx != nullptr && values != nullptr && out != nullptr, "sar_frame_gather_f32: null operand");
  SAR_REQUIRE(N >= 1 && C >= 1 && T >= 1 && V >= 1 && k >= 1 && k <= T, "sar_frame_gather_f32: bad sizes N=%d C=%d T=%d V=%d k=%d", N, C, T,
              V, k);
  const int64_t total = (int64_t)N * C * k * V;
  SAR_REQUIRE((int64_t)N * C * T * V < ((int64_t)1 << 40) && (total + 255) / 256 < ((int64_t)1 << 31), "sar_frame_gather_f32: tensor too large");
  frame_gather_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(s)>>>(x, idx, values, out, C, T, V, k, total);
  SAR_LAUNCH_CHECK("sar_frame_gather_f32");
  return 0;
}

// ---- the gather's gradients, one wave per (n, t): j = inv[n, t] names the output frame this frame went to (or -1).
//   dvalues[n, j] = sum_{c, v} dout[n, c, j, v] x[n, c, t, v]  (lane l adds elements l, l + 64, .. in order, then the xor tree)
//   dscores[n, t] = dvalues[n, j], 0 for a frame that was not chosen;  dx[n, c, t, v] = dout[n, c, j, v] values[n, j], 0 likewise
// Every element of the three outputs is written exactly once.
__global__ __launch_bounds__(256) void frame_gather_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                               const float* __restrict__ values, const int32_t* __restrict__ inv,
                                                               float* __restrict__ dvalues, float* __restrict__ dscores, int64_t sn,
                                                               int64_t st, float* __restrict__ dx, int N, int C, int T, int V, int k) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (int64_t)N * T) return;
  const int64_t n = w / T;
  const int t = (int)(w % T), CV = C * V;
  const int j = inv[w];
  if (j < 0 || j >= k) {
    if (lane == 0) dscores[n * sn + (int64_t)t * st] = 0.f;
    if (dx != nullptr)
      for (int i = lane; i < CV; i += 64) dx[((n * C + i / V) * T + t) * V + i % V] = 0.f;
    return;
  }
  const float val = values[n * k + j];
  float acc = 0.f;
  for (int i = lane; i < CV; i += 64) {
    const int c = i / V, v = i % V;
    const float d = dout[((n * C + c) * k + j) * V + v];
    const int64_t xi = ((n * C + c) * T + t) * V + v;
    acc = fmaf(d, x[xi], acc);
    if (dx != nullptr) dx[xi] = d * val;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    dvalues[n * k + j] = acc;
    dscores[n * sn + (int64_t)t * st] = acc;
  }
}

extern "C" int sar_frame_gather_bwd_f32(const float* x, const float* dout, const float* values, const int32_t* inv, float* dvalues,
                                        float* dscores, int64_t stride_n, int64_t stride_t, float* dx, int N, int C, int T, int V, int k,
                                        sar_stream_t s) {
  SAR_REQUIRE(x != nullptr && dout != nullptr && values != nullptr && inv != nullptr && dvalues != nullptr && dscores != nullptr,
              "sar_frame_gather_bwd_f32: null operand");
  SAR_REQUIRE(N >= 1 && C >= 1 && T >= 1 && V >= 1 && k >= 1 && k <= T && stride_n >= 1 && stride_t >= 1,
              "sar_frame_gather_bwd_f32: bad sizes N=%d C=%d T=%d V=%d k=%d", N, C, T, V, k);
  SAR_REQUIRE((int64_t)C * V < ((int64_t)1 << 30) && (int64_t)N * T < ((int64_t)1 << 31) && (int64_t)N * C * T * V < ((int64_t)1 << 40),
              "sar_frame_gather_bwd_f32: tensor too large");
  frame_gather_bwd_kernel<<<(unsigned)(((int64_t)N * T + 3) / 4), 256, 0, as_stream(s)>>>(x, dout, values, inv, dvalues, dscores, stride_n,
                                                                                          stride_t, dx, N, C, T, V, k);
  SAR_LAUNCH_CHECK("sar_frame_gather_bwd_f32");
  return 0;
}

// ---- (N, C, T, V) <-> the stack's input matrix X[v C + c][t N + n] (x_lstm[n, t, v C + c] of models/lstm_sampler.py:17-18), through an
// LDS tile of 64 sequences x 32 joints of one (c, t): runs of V floats on the NCHW side, runs of 64 on the CN side.
// ADD = false: X = pack(x).  ADD = true: x += unpack(X) (the LSTM-path input gradient added into the gather-path one).
template <bool ADD>
__global__ __launch_bounds__(256) void lstm_pack_kernel(float* __restrict__ x, float* __restrict__ X, int64_t ld, int N, int C, int T, int V) {
  __shared__ float tile[PACK_NT][PACK_VT + 1];
  const int n0 = blockIdx.x * PACK_NT, t = blockIdx.y, c = blockIdx.z, tid = threadIdx.x;
  for (int v0 = 0; v0 < V; v0 += PACK_VT) {
    if (!ADD) {
      for (int i = tid; i < PACK_NT * PACK_VT; i += 256) {
        const int nn = i / PACK_VT, vv = i % PACK_VT;
        if (n0 + nn < N && v0 + vv < V) tile[nn][vv] = x[(((int64_t)(n0 + nn) * C + c) * T + t) * V + v0 + vv];
      }
      __syncthreads();
      for (int i = tid; i < PACK_NT * PACK_VT; i += 256) {
        const int vv = i / PACK_NT, nn = i % PACK_NT;
        if (n0 + nn < N && v0 + vv < V) X[((int64_t)(v0 + vv) * C + c) * ld + (int64_t)t * N + n0 + nn] = tile[nn][vv];
      }
    } else {
      for (int i = tid; i < PACK_NT * PACK_VT; i += 256) {
        const int vv = i / PACK_NT, nn = i % PACK_NT;
        if (n0 + nn < N && v0 + vv < V) tile[nn][vv] = X[((int64_t)(v0 + vv) * C + c) * ld + (int64_t)t * N + n0 + nn];
      }
      __syncthreads();
      for (int i = tid; i < PACK_NT * PACK_VT; i += 256) {
        const int nn = i / PACK_VT, vv = i % PACK_VT;
        if (n0 + nn < N && v0 + vv < V) x[(((int64_t)(n0 + nn) * C + c) * T + t) * V + v0 + vv] += tile[nn][vv];
      }
    }
    __syncthreads();      // the tile is rewritten by the next joint chunk
  }
}

static int lstm_pack_check(const char* name, const void* x, const void* X, int64_t ld, int N, int C, int T, int V) {
  SAR_REQUIRE(x != nullptr && X != nullptr, "%s: null operand", name);
  SAR_REQUIRE(N >= 1 && C >= 1 && T >= 1 && V >= 1, "%s: bad sizes N=%d C=%d T=%d V=%d", name, N, C, T, V);
  SAR_REQUIRE((int64_t)T * N < ((int64_t)1 << 31) && ld >= (int64_t)T * N, "%s: leading dimension smaller than T*N (or T*N >= 2^31)", name);
  SAR_REQUIRE(T <= 65535 && C <= 65535 && (int64_t)C * V < ((int64_t)1 << 24), "%s: built for T, C <= 65535 and C*V < 2^24", name);
  return 0;
}

extern "C" int sar_lstm_pack_f32(const float* x, float* X, int64_t ld, int N, int C, int T, int V, sar_stream_t s) {
  if (int rc = lstm_pack_check("sar_lstm_pack_f32", x, X, ld, N, C, T, V)) return rc;
  const dim3 grid((unsigned)((N + PACK_NT - 1) / PACK_NT), (unsigned)T, (unsigned)C);
  lstm_pack_kernel<false><<<grid, 256, 0, as_stream(s)>>>(const_cast<float*>(x), X, ld, N, C, T, V);
  SAR_LAUNCH_CHECK("sar_lstm_pack_f32");
  return 0;
}

extern "C" int sar_lstm_unpack_add_f32(const float* X, int64_t ld, float* x, int N, int C, int T, int V, sar_stream_t s) {
  if (int rc = lstm_pack_check("sar_lstm_unpack_add_f32", x, X, ld, N, C, T, V)) return rc;
  const dim3 grid((unsigned)((N + PACK_NT - 1) / PACK_NT), (unsigned)T, (unsigned)C);
  lstm_pack_kernel<true><<<grid, 256, 0, as_stream(s)>>>(x, const_cast<float*>(X), ld, N, C, T, V);
  SAR_LAUNCH_CHECK("sar_lstm_unpack_add_f32");
  return 0;
}
