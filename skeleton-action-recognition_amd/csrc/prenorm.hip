// prenorm.hip -- the reference's data_gen/preprocess.py:8-88 `pre_normalization(data, zaxis, xaxis)` (with data_gen/rotation.py:5-42)
// as ONE pass over a batch of raw skeleton clips (N, 3, T, V, M) fp32 -> a separate output of the same shape:
//   pad     per non-null body: frame 0 null -> the non-null frames move to the front in order; L = one past the last non-null frame;
//           frames t >= L become frame (t - L) mod L.  Null frames before L (interior gaps) stay null.  (preprocess.py:13-32)
//   centre  unless every body of the clip is null: every non-null body minus body 0's joint 1 of the same (padded) frame, in fp32,
//           times the joint's own not-null mask (a dropped joint stays 0).  Joint 1 is hard-coded as in preprocess.py:40.
//   rot z   one matrix per clip from body 0, frame 0, joints zaxis[0] -> zaxis[1] AFTER centring: the difference and its unit vector
//           in fp32, cross product, arccos, the Euler-Rodrigues matrix and the product with the fp32 joint in fp64, rounded to fp32.
//   rot x   the same from joints xaxis[0], xaxis[1] of the fp32-ROUNDED output of the z rotation and (1, 0, 0).  The two matrices
//           are NOT merged: the intermediate rounding is part of the result.
// Identity branches (rotation.py:10, :38): angle_between returns 0 when sum|v| < 1e-6; rotation_matrix returns the identity when
// sum|axis| < 1e-6 or |theta| < 1e-6 -- so a bone already on its axis AND an antiparallel bone (cross product 0) are left alone.
// "Null" here means ALL coordinates EXACTLY zero.  The reference tests x.sum() == 0, which differs only under exact cancellation.
// The reference skips the rotation of null frames / bodies; a rotation maps zeros to zeros, so nothing is skipped here.
//
// One workgroup of 1024 lanes per clip; nothing in a clip's result depends on another clip; no atomics.
//   phase A  one coalesced sweep sets flag[m][t] = 1 in LDS for every frame with a non-zero coordinate (lanes store the same byte);
//            wave m then turns body m's flags into src[m][t], the source frame of padded frame t, with ballot prefix counts
//   phase B  lane 0: the two matrices from four joints of body 0's frame 0, in double, broadcast through LDS
//   phase C  one streaming sweep along the contiguous (V, M) rows: gather frame src[m][t], centre, mask, rotate twice, store
// The sweeps issue four independent loads per lane before the first use: a clip is one workgroup's latency chain, not bandwidth.
#include "sar_common.h"

#define PN_THREADS 1024
#define PN_UNROLL 4
#define PN_MAX_T 2048
#define PN_MAX_V 32
#define PN_MAX_M 4

// rotation.py:28-42 + :5-20 for v (fp32) and the unit target axis e_k (k = 2: z, k = 0: x); R row-major
__device__ void pn_matrix(const float v[3], int k, double R[9]) {
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  const float s1 = (fabsf(v[0]) + fabsf(v[1])) + fabsf(v[2]);
  if (s1 < 1e-6f) return;                                   // angle_between -> 0 -> rotation_matrix -> identity
  const float nrm = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  double c = (double)(v[k] / nrm);                          // dot(unit(v), e_k): the other two products are exact zeros
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  const double theta = acos(c);
  // np.cross(v, e_k) in double: e_z -> (v1, -v0, 0), e_x -> (0, v2, -v1)
  double ax[3];
  if (k == 2) ax[0] = (double)v[1], ax[1] = -(double)v[0], ax[2] = 0.0;
  else ax[0] = 0.0, ax[1] = (double)v[2], ax[2] = -(double)v[1];
  if (fabs(ax[0]) + fabs(ax[1]) + fabs(ax[2]) < 1e-6 || fabs(theta) < 1e-6) return;
  const double inv = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  const double a = cos(theta / 2.0), sn = sin(theta / 2.0);
  const double b = -(ax[0] / inv) * sn, cc_ = -(ax[1] / inv) * sn, d = -(ax[2] / inv) * sn;
  const double aa = a * a, bb = b * b, cc = cc_ * cc_, dd = d * d;
  const double bc = b * cc_, ad = a * d, ac = a * cc_, ab = a * b, bd = b * d, cd = cc_ * d;
  R[0] = aa + bb - cc - dd, R[1] = 2 * (bc + ad), R[2] = 2 * (bd - ac);
  R[3] = 2 * (bc - ad), R[4] = aa + cc - bb - dd, R[5] = 2 * (cd + ab);
  R[6] = 2 * (bd + ac), R[7] = 2 * (cd - ab), R[8] = aa + dd - bb - cc;
}

// np.dot(float64 matrix, fp32 joint) rounded to fp32
__device__ __forceinline__ void pn_rotate(const double* R, float& x, float& y, float& z) {
  const double dx = x, dy = y, dz = z;
  x = (float)(R[0] * dx + R[1] * dy + R[2] * dz);
  y = (float)(R[3] * dx + R[4] * dy + R[5] * dz);
  z = (float)(R[6] * dx + R[7] * dy + R[8] * dz);
}

__global__ __launch_bounds__(PN_THREADS) void prenorm_kernel(const float* __restrict__ x, float* __restrict__ out, int T, int V, int M,
                                                             int z0, int z1, int x0, int x1) {
  __shared__ unsigned char flag[PN_MAX_M * PN_MAX_T];
  __shared__ unsigned short src[PN_MAX_M * PN_MAX_T];
  __shared__ int nvalid[PN_MAX_M];
  __shared__ double rot[18];
  const int tid = threadIdx.x, VM = V * M, P = T * VM;
  const float* xc = x + (int64_t)blockIdx.x * 3 * P;
  float* oc = out + (int64_t)blockIdx.x * 3 * P;

  // ---- phase A: null flags
  for (int i = tid; i < M * T; i += PN_THREADS) flag[i] = 0;
  __syncthreads();
  for (int e0 = tid; e0 < P; e0 += PN_THREADS * PN_UNROLL) {
    float a[PN_UNROLL][3];
#pragma unroll
    for (int u = 0; u < PN_UNROLL; ++u) {
      const int e = e0 + u * PN_THREADS;
#pragma unroll
      for (int c = 0; c < 3; ++c) a[u][c] = e < P ? xc[c * P + e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < PN_UNROLL; ++u) {
      const int e = e0 + u * PN_THREADS;
      if (a[u][0] != 0.f || a[u][1] != 0.f || a[u][2] != 0.f) flag[(e % M) * T + e / VM] = 1;   // e < P: the padding lanes hold zeros
    }
  }
  __syncthreads();
  // wave m: src[m][t].  keep(t) = the frames that stay, in order: the non-null ones when frame 0 is null (compaction), else 0 .. L-1
  const int wave = tid >> 6, lane = tid & 63;
  if (wave < M) {
    const unsigned char* f = flag + wave * T;
    unsigned short* sr = src + wave * T;
    int cnt = 0, last = -1;
    for (int b = 0; b < T; b += 64) {
      const bool on = b + lane < T && f[b + lane] != 0;
      const unsigned long long mask = __ballot(on);
      cnt += __popcll(mask);
      if (mask) last = b + 63 - __clzll(mask);
    }
    const bool compact = cnt > 0 && f[0] == 0;
    const int L = cnt == 0 ? T : (compact ? cnt : last + 1);
    if (compact) {
      int run = 0;
      for (int b = 0; b < T; b += 64) {
        const bool on = b + lane < T && f[b + lane] != 0;
        const unsigned long long mask = __ballot(on);
        if (on) sr[run + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)(b + lane);
        run += __popcll(mask);
      }
    } else {
      for (int t = lane; t < L; t += 64) sr[t] = (unsigned short)t;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int t = L + lane; t < T; t += 64) sr[t] = sr[(t - L) % L];      // reads entries < L only, which this loop never writes
    if (lane == 0) nvalid[wave] = cnt;
  }
  __syncthreads();

  // ---- phase B: the two matrices (body 0, padded frame 0)
  if (tid == 0) {
    const int f0 = src[0];
    float j[4][3], ctr[3];
    const int joints[4] = {z0, z1, x0, x1};
    for (int c = 0; c < 3; ++c) ctr[c] = xc[c * P + f0 * VM + 1 * M];
    for (int q = 0; q < 4; ++q) {
      float p[3];
      for (int c = 0; c < 3; ++c) p[c] = xc[c * P + f0 * VM + joints[q] * M];
      const bool nz = p[0] != 0.f || p[1] != 0.f || p[2] != 0.f;          // body 0 null: all zeros, the matrices are identities
      for (int c = 0; c < 3; ++c) j[q][c] = nz ? p[c] - ctr[c] : 0.f;
    }
    double Rz[9], Rx[9];
    const float dz[3] = {j[1][0] - j[0][0], j[1][1] - j[0][1], j[1][2] - j[0][2]};
    pn_matrix(dz, 2, Rz);
    pn_rotate(Rz, j[2][0], j[2][1], j[2][2]);
    pn_rotate(Rz, j[3][0], j[3][1], j[3][2]);
    const float dx[3] = {j[2][0] - j[3][0], j[2][1] - j[3][1], j[2][2] - j[3][2]};
    pn_matrix(dx, 0, Rx);
    for (int i = 0; i < 9; ++i) rot[i] = Rz[i], rot[9 + i] = Rx[i];
  }
  __syncthreads();
  double Rz[9], Rx[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rz[i] = rot[i], Rx[i] = rot[9 + i];

  // ---- phase C: gather, centre, mask, rotate, store
  for (int e0 = tid; e0 < P; e0 += PN_THREADS * PN_UNROLL) {
    float a[PN_UNROLL][3], ctr[PN_UNROLL][3];
    bool body[PN_UNROLL];
#pragma unroll
    for (int u = 0; u < PN_UNROLL; ++u) {
      const int e = e0 + u * PN_THREADS;
      body[u] = false;
      if (e < P) {
        const int t = e / VM, r = e - t * VM, m = r % M;
        body[u] = nvalid[m] > 0;
        const int fs = src[m * T + t] * VM + r, fc = src[t] * VM + M;     // a null body keeps src = t; body 0's joint 1
#pragma unroll
        for (int c = 0; c < 3; ++c) a[u][c] = xc[c * P + fs], ctr[u][c] = xc[c * P + fc];
      }
    }
#pragma unroll
    for (int u = 0; u < PN_UNROLL; ++u) {
      const int e = e0 + u * PN_THREADS;
      if (e >= P) continue;
      float px = 0.f, py = 0.f, pz = 0.f;
      if (body[u] && (a[u][0] != 0.f || a[u][1] != 0.f || a[u][2] != 0.f)) {
        px = a[u][0] - ctr[u][0], py = a[u][1] - ctr[u][1], pz = a[u][2] - ctr[u][2];
        pn_rotate(Rz, px, py, pz);
        pn_rotate(Rx, px, py, pz);
      }
      oc[e] = px, oc[P + e] = py, oc[2 * P + e] = pz;
    }
  }
}

extern "C" int sar_pre_normalize_f32(const float* x, float* out, int N, int T, int V, int M, int z0, int z1, int x0, int x1,
                                     sar_stream_t s) {
  SAR_REQUIRE(x != nullptr && out != nullptr && N >= 0 && T >= 1 && V >= 1 && M >= 1, "sar_pre_normalize_f32: bad arguments");
  if (V < 2 || V > PN_MAX_V || M > PN_MAX_M || T > PN_MAX_T) {
    sar_set_error("sar_pre_normalize_f32: built for 2 <= V <= %d, M <= %d, T <= %d (got V %d M %d T %d)", PN_MAX_V, PN_MAX_M, PN_MAX_T,
                  V, M, T);
    return SAR_E_UNSUP;
  }
  SAR_REQUIRE(z0 >= 0 && z0 < V && z1 >= 0 && z1 < V && x0 >= 0 && x0 < V && x1 >= 0 && x1 < V,
              "sar_pre_normalize_f32: joint index outside [0, V)");
  if (N == 0) return 0;
  const uintptr_t bytes = (uintptr_t)N * 3 * T * V * M * sizeof(float), xa = (uintptr_t)x, oa = (uintptr_t)out;
  SAR_REQUIRE(xa + bytes <= oa || oa + bytes <= xa, "sar_pre_normalize_f32: out must not overlap x (frames are gathered)");
  prenorm_kernel<<<(unsigned)N, PN_THREADS, 0, as_stream(s)>>>(x, out, T, V, M, z0, z1, x0, x1);
  SAR_LAUNCH_CHECK("sar_pre_normalize_f32");
  return 0;
}
