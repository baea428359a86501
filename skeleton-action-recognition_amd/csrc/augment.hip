// augment.hip -- training-time augmentation of a batch of skeleton clips (N, 3, T, V, M) fp32 -> a separate output of the same shape,
// ONE launch: a per-clip temporal crop-resize, then a per-frame rotation, scale and shift whose parameters move linearly from a
// start key frame to an end key frame.  The random numbers are the host's (sar_amd/augment.py): the kernel applies one row
//   params[n] = [p, o, a0, b0, g0, s0, dx0, dy0, dz0, a1, b1, g1, s1, dx1, dy1, dz1]            (fp32)
// per clip and is a pure function of (x, params, crop).  The contract (DESIGN.md "Augmentation"; tests/augment_reference.py):
//   1  L = one past the last frame with a non-zero coordinate ("null" = all coordinates exactly zero, as in prenorm.hip); L = 0 ->
//      the clip is zero.  crop == 0: L := T, p := 1, o := 0 (identity time map, padding kept).
//   2  Lc = max(1, floor(p L)), b = min(floor(o (L - Lc + 1)), L - Lc), the products in double.  (Both are also clamped into
//      [1, L] and [0, L - Lc]: a row outside the documented ranges, or NaN, cannot move a read out of the clip.)
//   3  output frame t reads s = clamp((t + 0.5) Lc / T - 0.5, 0, Lc - 1) in double, i0 = floor(s), i1 = min(i0 + 1, Lc - 1),
//      w = fp32(s - i0); the source frames are b + i0, b + i1  (linear, half-pixel centres; Lc = T gives w = 0 exactly).
//   4  per joint: near = the source frame closer to s (i0 on a tie), far = the other.  near null -> (0, 0, 0), nothing else applied;
//      far null -> u = the near joint; else u = (1 - w) x[i0] + w x[i1] in fp32.  (w = 0 takes x[i0] itself: the same value, and
//      the sign of a zero coordinate survives.)
//   5  tau = t / (T - 1) (0 when T = 1); every parameter a(tau) = a0 + tau (a1 - a0) in double; R = Rz(g) Ry(b) Rx(a) in double, its
//      nine entries rounded to fp32; out = s (R u) + d in fp32.  A frame whose fp32 R, s, d are exactly I, 1, 0 copies u.
//   6  hence p = 1, o = 0, zero angles and shifts, unit scales, no trailing null frames: out is bitwise x.
//
// One workgroup of 1024 lanes per clip; nothing in a clip's result depends on another clip; no atomics.
//   phase A  (crop only) one coalesced sweep sets flag[t] = 1 in LDS for every frame with a non-zero coordinate (lanes store the same
//            byte); wave 0 turns the flags into L with ballots
//   phase B  per chunk of AG_CHUNK output frames: lane j builds frame j's 16-word record (R, s, d, w, i0, flags) in LDS -- the only
//            double-precision arithmetic and the only trigonometry of the kernel, once per frame instead of once per coordinate
//   phase C  one streaming sweep along the contiguous (V, M) rows of the chunk: the three channels of BOTH source frames of four
//            elements are loaded before the first use (a clip is one workgroup's latency chain), blended, rotated, stored
// T = 300 is one chunk (19 KB of records); the T limit of 2048 is four.
#include "sar_common.h"

#define AG_THREADS 1024
#define AG_UNROLL 4
#define AG_CHUNK 512
#define AG_MAX_T 2048
#define AG_MAX_V 32
#define AG_MAX_M 4
#define AG_NEAR_I1 1       // record flags: the nearer source frame is b + i1
#define AG_PLAIN 2         //               R, s, d are exactly I, 1, 0: the frame copies u
#define AG_STEP 4          //               i1 = i0 + 1 (else i1 = i0)

// floor(v) clamped into [lo, hi]; NaN -> lo
__device__ __forceinline__ int ag_floor_clamp(double v, int lo, int hi) {
  v = floor(v);
  return !(v >= (double)lo) ? lo : (v > (double)hi ? hi : (int)v);
}

__global__ __launch_bounds__(AG_THREADS) void augment_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                             float* __restrict__ out, int T, int V, int M, int crop) {
  __shared__ float4 tab[AG_CHUNK * 4];
  __shared__ unsigned char flag[AG_MAX_T];
  __shared__ int valid;
  const int tid = threadIdx.x, VM = V * M, P = T * VM;
  const float* xc = x + (int64_t)blockIdx.x * 3 * P;
  float* oc = out + (int64_t)blockIdx.x * 3 * P;
  const float* pr = params + (int64_t)blockIdx.x * 16;

  // ---- phase A: the valid length
  int L = T;
  if (crop) {
    for (int i = tid; i < T; i += AG_THREADS) flag[i] = 0;
    __syncthreads();
    for (int e0 = tid; e0 < P; e0 += AG_THREADS * AG_UNROLL) {
      float a[AG_UNROLL][3];
#pragma unroll
      for (int u = 0; u < AG_UNROLL; ++u) {
        // past the end: the last element once more (the same flag) -- the twelve loads are unconditional and in flight together
        const int e = min(e0 + u * AG_THREADS, P - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) a[u][c] = xc[c * P + e];
      }
#pragma unroll
      for (int u = 0; u < AG_UNROLL; ++u) {
        const int e = min(e0 + u * AG_THREADS, P - 1);
        if (a[u][0] != 0.f || a[u][1] != 0.f || a[u][2] != 0.f) flag[e / VM] = 1;
      }
    }
    __syncthreads();
    if (tid < 64) {
      int last = -1;
      for (int b = 0; b < T; b += 64) {
        const unsigned long long mask = __ballot(b + tid < T && flag[b + tid] != 0);
        if (mask) last = b + 63 - __clzll(mask);
      }
      if (tid == 0) valid = last + 1;
    }
    __syncthreads();
    L = valid;
    if (L == 0) {                                            // the same in every lane: no barrier follows for anyone
      for (int e = tid; e < 3 * P; e += AG_THREADS) oc[e] = 0.f;
      return;
    }
  }

  // ---- the crop window (every lane, the same values)
  const double p = crop ? (double)pr[0] : 1.0, o = crop ? (double)pr[1] : 0.0;
  const int Lc = ag_floor_clamp(p * (double)L, 1, L);
  const int b = ag_floor_clamp(o * (double)(L - Lc + 1), 0, L - Lc);

  for (int t0 = 0; t0 < T; t0 += AG_CHUNK) {
    const int nt = min(AG_CHUNK, T - t0);
    if (t0) __syncthreads();                                 // the previous chunk's sweep has read its records
    // ---- phase B: the records of frames t0 .. t0 + nt - 1
    if (tid < nt) {
      const int t = t0 + tid;
      double s = ((double)t + 0.5) * (double)Lc / (double)T - 0.5;
      s = s < 0.0 ? 0.0 : (s > (double)(Lc - 1) ? (double)(Lc - 1) : s);
      const int i0 = (int)floor(s);
      const double fr = s - (double)i0;
      const int step = i0 + 1 <= Lc - 1 ? 1 : 0;
      const double tau = T > 1 ? (double)t / (double)(T - 1) : 0.0;
      double q[7];                                           // alpha, beta, gamma, scale, dx, dy, dz at tau
#pragma unroll
      for (int i = 0; i < 7; ++i) q[i] = (double)pr[2 + i] + tau * ((double)pr[9 + i] - (double)pr[2 + i]);
      const double sa = sin(q[0]), ca = cos(q[0]), sb = sin(q[1]), cb = cos(q[1]), sg = sin(q[2]), cg = cos(q[2]);
      float R[9];
      R[0] = (float)(cb * cg), R[1] = (float)(sa * sb * cg - ca * sg), R[2] = (float)(ca * sb * cg + sa * sg);
      R[3] = (float)(cb * sg), R[4] = (float)(sa * sb * sg + ca * cg), R[5] = (float)(ca * sb * sg - sa * cg);
      R[6] = (float)(-sb), R[7] = (float)(sa * cb), R[8] = (float)(ca * cb);
      const float sc = (float)q[3], dx = (float)q[4], dy = (float)q[5], dz = (float)q[6];
      bool plain = sc == 1.f && dx == 0.f && dy == 0.f && dz == 0.f;
#pragma unroll
      for (int i = 0; i < 9; ++i) plain = plain && R[i] == (i % 4 == 0 ? 1.f : 0.f);
      const int fl = (fr > 0.5 ? AG_NEAR_I1 : 0) | (plain ? AG_PLAIN : 0) | (step ? AG_STEP : 0);
      tab[tid * 4 + 0] = make_float4(R[0], R[1], R[2], R[3]);
      tab[tid * 4 + 1] = make_float4(R[4], R[5], R[6], R[7]);
      tab[tid * 4 + 2] = make_float4(R[8], sc, dx, dy);
      tab[tid * 4 + 3] = make_float4(dz, (float)fr, __int_as_float(i0), __int_as_float(fl));
    }
    __syncthreads();

    // ---- phase C: gather two source frames, blend, rotate, scale, shift, store
    const int e_end = (t0 + nt) * VM;
    for (int e0 = t0 * VM + tid; e0 < e_end; e0 += AG_THREADS * AG_UNROLL) {
      float a0[AG_UNROLL][3], a1[AG_UNROLL][3];
      int rec[AG_UNROLL];
#pragma unroll
      for (int u = 0; u < AG_UNROLL; ++u) {
        const int e = e0 + u * AG_THREADS;
        rec[u] = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) a0[u][c] = a1[u][c] = 0.f;
        if (e < e_end) {
          const int t = e / VM, r = e - t * VM;
          rec[u] = (t - t0) * 4;
          const float4 h = tab[rec[u] + 3];
          // b + i0 <= b + i1 <= b + Lc - 1 <= L - 1 <= T - 1: both reads stay inside the clip
          const int f0 = (b + __float_as_int(h.z)) * VM + r, f1 = f0 + ((__float_as_int(h.w) & AG_STEP) ? VM : 0);
#pragma unroll
          for (int c = 0; c < 3; ++c) a0[u][c] = xc[c * P + f0], a1[u][c] = xc[c * P + f1];
        }
      }
#pragma unroll
      for (int u = 0; u < AG_UNROLL; ++u) {
        const int e = e0 + u * AG_THREADS;
        if (e >= e_end) continue;
        const float4 r0 = tab[rec[u]], r1 = tab[rec[u] + 1], r2 = tab[rec[u] + 2], r3 = tab[rec[u] + 3];
        const float w = r3.y;
        const int fl = __float_as_int(r3.w);
        const bool n0 = a0[u][0] == 0.f && a0[u][1] == 0.f && a0[u][2] == 0.f;
        const bool n1 = a1[u][0] == 0.f && a1[u][1] == 0.f && a1[u][2] == 0.f;
        const bool near1 = (fl & AG_NEAR_I1) != 0;
        const bool near_null = near1 ? n1 : n0, far_null = near1 ? n0 : n1;
        const bool blend = !far_null && w != 0.f;
        float uu[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float nearv = near1 ? a1[u][c] : a0[u][c];
          uu[c] = blend ? (1.f - w) * a0[u][c] + w * a1[u][c] : nearv;
        }
        float px = uu[0], py = uu[1], pz = uu[2];
        if (!(fl & AG_PLAIN)) {
          px = r2.y * (r0.x * uu[0] + r0.y * uu[1] + r0.z * uu[2]) + r2.z;
          py = r2.y * (r0.w * uu[0] + r1.x * uu[1] + r1.y * uu[2]) + r2.w;
          pz = r2.y * (r1.z * uu[0] + r1.w * uu[1] + r2.x * uu[2]) + r3.x;
        }
        if (near_null) px = py = pz = 0.f;
        oc[e] = px, oc[P + e] = py, oc[2 * P + e] = pz;
      }
    }
  }
}

extern "C" int sar_augment_clips_f32(const float* x, const float* params, float* out, int N, int T, int V, int M, int crop,
                                     sar_stream_t s) {
  SAR_REQUIRE(x != nullptr && params != nullptr && out != nullptr && N >= 0 && T >= 1 && V >= 1 && M >= 1,
              "sar_augment_clips_f32: bad arguments");
  if (V > AG_MAX_V || M > AG_MAX_M || T > AG_MAX_T) {
    sar_set_error("sar_augment_clips_f32: built for V <= %d, M <= %d, T <= %d (got V %d M %d T %d)", AG_MAX_V, AG_MAX_M, AG_MAX_T, V, M,
                  T);
    return SAR_E_UNSUP;
  }
  if (N == 0) return 0;
  const uintptr_t bytes = (uintptr_t)N * 3 * T * V * M * sizeof(float), pbytes = (uintptr_t)N * 16 * sizeof(float);
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out, pa = (uintptr_t)params;
  SAR_REQUIRE(xa + bytes <= oa || oa + bytes <= xa, "sar_augment_clips_f32: out must not overlap x (frames are gathered)");
  SAR_REQUIRE(pa + pbytes <= oa || oa + bytes <= pa, "sar_augment_clips_f32: out must not overlap params");
  augment_kernel<<<(unsigned)N, AG_THREADS, 0, as_stream(s)>>>(x, params, out, T, V, M, crop != 0);
  SAR_LAUNCH_CHECK("sar_augment_clips_f32");
  return 0;
}
