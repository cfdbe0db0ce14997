// The text-to-motion metric kernels (engine/path_metrics.hpp; mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist): the device-shaped parts of
// TM2TMetrics and MMMetrics on embeddings [N][D] that stay on the device.
//
// Replaces: the group loop of TM2TMetrics.compute (mld/models/metrics/tm2t.py:100-134: euclidean_distance_matrix, nan_to_num, trace, argsort,
// calculate_top_k), calculate_activation_statistics_np and the distance part of calculate_diversity_np / calculate_multimodality_np
// (mld/models/metrics/utils.py).  include/mldhip.h has the math and the rules.
//
// Exact fp32 in every precision mode: v_mfma_f32_16x16x4_f32 for the products, fp32 VALU elsewhere.  No atomics; every sum has one fixed order.
//
// t2m_match_kernel: ONE workgroup per group of R <= 32 rows; the 32 x 32 distance tile is four 16 x 16 MFMA tiles, one per wave.  K = D goes through LDS
//   in slabs of 128 (rows behind R and columns behind D are zeros); a lane reads 8 consecutive k of its row per 32-wide chunk (lane group g of MFMA i
//   takes k = 8 g + i: the A and B operands agree, so the products are the same sums), two accumulator chains.  The squared norms come from the same
//   slabs: four lanes per row, k = q mod 4, combined (s0 + s1) + (s2 + s3).  The rank of the diagonal is counted by one lane per row.
// act_mean_kernel: 64 columns per workgroup, four lanes per column; lane q sums chunks q, q + 4, ... (compensated sums, rows of a chunk in order, chunk
//   sums in order), the four partial sums are combined (s0 + s1) + (s2 + s3).
// act_cov_kernel: ONE workgroup per upper 32 x 32 tile (ti <= tj) of the covariance.  Rows are centred while they are staged (x - mean, 128 rows per
//   slab); a chunk of MLDHIP_ACT_STATS_CHUNK = 256 rows is summed from zero by MFMAs (K = rows), the chunk sums are added in ascending order.  Only
//   elements i <= j are stored, each to [i][j] and [j][i].  No workspace: the chunk sums never leave the registers.
// pair_dist_kernel: one wave per pair; lane l takes d = l mod 64.
#pragma once
#include <cfloat>
#include "rt.hpp"

namespace mld {

constexpr int kMetMaxD = 1024, kMetR = 32;
constexpr int kMetKC = 128, kMetKS = kMetKC + 4;      // K slab of the match kernel and its LDS row stride (16 rows x 16-byte reads land on distinct banks)
constexpr int kStatChunk = 256;                        // MLDHIP_ACT_STATS_CHUNK
constexpr int kStatStage = 128, kStatLd = 48;          // rows per staged slab; LDS row stride (the four lane groups of an operand read hit distinct banks)

struct MatchArgs {
  const float* text;      // [N][D]
  const float* motion;    // [N][D]
  int* rank;              // [G R] or NULL
  float* diag;            // [G R] or NULL
  int D, R;
};

// grid G, block 256
__global__ __launch_bounds__(256) void t2m_match_kernel(MatchArgs p) {
  __shared__ __attribute__((aligned(16))) float ts[kMetR * kMetKS];
  __shared__ __attribute__((aligned(16))) float ms[kMetR * kMetKS];
  __shared__ float dist[kMetR * (kMetR + 1)];
  __shared__ float nrm[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int col = lane & 15, grp = lane >> 4;
  const int ti = wave >> 1, tj = wave & 1;
  const long long row0 = (long long)blockIdx.x * p.R;
  const int nrow = tid >> 2, nq = tid & 3;              // norm of row nrow (0 .. 31 text, 32 .. 63 motion), k = nq mod 4
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float ns = 0.f;
  for (int k0 = 0; k0 < p.D; k0 += kMetKC) {
    for (int i = tid; i < 2 * kMetR * kMetKC; i += 256) {
      const int r = i / kMetKC, k = i % kMetKC, rr = r & (kMetR - 1);
      float v = 0.f;
      if (rr < p.R && k0 + k < p.D) v = (r < kMetR ? p.text : p.motion)[(row0 + rr) * p.D + k0 + k];
      (r < kMetR ? ts : ms)[rr * kMetKS + k] = v;
    }
    __syncthreads();
    const int left = p.D - k0;
    const int kend = left >= kMetKC ? kMetKC : (left + 31) & ~31;      // (uniform; the slab is zero behind D)
    {
      const float* src = (nrow < kMetR ? ts : ms) + (nrow & (kMetR - 1)) * kMetKS;
      for (int k = nq; k < kend; k += 4) ns = fmaf(src[k], src[k], ns);
    }
    const float* ar = ts + (ti * 16 + col) * kMetKS + 8 * grp;
    const float* br = ms + (tj * 16 + col) * kMetKS + 8 * grp;
    for (int kc = 0; kc < kend; kc += 32) {
      const F4 al = ld4(ar + kc), ah = ld4(ar + kc + 4), bl = ld4(br + kc), bh = ld4(br + kc + 4);
      const float a[8] = {al.x, al.y, al.z, al.w, ah.x, ah.y, ah.z, ah.w};
      const float b[8] = {bl.x, bl.y, bl.z, bl.w, bh.x, bh.y, bh.z, bh.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i & 1] = mfma_f32_16x16x4(a[i], b[i], acc[i & 1]);
    }
    __syncthreads();
  }
  nrm[tid] = ns;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ti * 16 + grp * 4 + r, j = tj * 16 + col;
    const float nt = (nrm[4 * i] + nrm[4 * i + 1]) + (nrm[4 * i + 2] + nrm[4 * i + 3]);
    const float nm = (nrm[4 * (kMetR + j)] + nrm[4 * (kMetR + j) + 1]) + (nrm[4 * (kMetR + j) + 2] + nrm[4 * (kMetR + j) + 3]);
    const float dot = acc[0][r] + acc[1][r];
    const float arg = (-2.f * dot + nt) + nm;            // d1 + d2 + d3 in the reference's order
    float d = arg >= 0.f ? sqrtf(arg) : 0.f;             // nan_to_num: a negative or NaN argument gives 0 ...
    if (d > FLT_MAX) d = FLT_MAX;                        // ... and +inf the largest finite value
    dist[i * (kMetR + 1) + j] = d;
  }
  __syncthreads();
  if (tid < p.R) {
    const float* row = dist + tid * (kMetR + 1);
    const float dii = row[tid];
    int cnt = 0;
    for (int j = 0; j < p.R; ++j) cnt += (row[j] < dii || (j < tid && row[j] == dii)) ? 1 : 0;
    if (p.rank) p.rank[row0 + tid] = cnt;
    if (p.diag) p.diag[row0 + tid] = dii;
  }
}

struct StatArgs {
  const float* x;      // [N][D]
  float* mean;         // [D]
  float* cov;          // [D][D]
  int N, D;
};

// compensated (Kahan) running sum: s is the sum, c the part of the last terms that did not fit
__device__ __forceinline__ void kahan_add(float& s, float& c, float v) {
  const float y = v - c, t = s + y;
  c = (t - s) - y;
  s = t;
}

// grid ceil(D / 64), block 256
__global__ __launch_bounds__(256) void act_mean_kernel(StatArgs p) {
  __shared__ float part[256];
  const int tid = threadIdx.x, q = tid >> 6, c = blockIdx.x * 64 + (tid & 63);
  const int nch = (p.N + kStatChunk - 1) / kStatChunk;
  float S = 0.f, C = 0.f;
  if (c < p.D) {
    for (int ch = q; ch < nch; ch += 4) {
      const int n0 = ch * kStatChunk, n1 = n0 + kStatChunk < p.N ? n0 + kStatChunk : p.N;
      const float* x = p.x + (long long)n0 * p.D + c;
      float s = 0.f, e = 0.f;
      for (int n = n0; n < n1; ++n, x += p.D) kahan_add(s, e, *x);
      kahan_add(S, C, s);
    }
  }
  part[tid] = S;
  __syncthreads();
  if (q == 0 && c < p.D) p.mean[c] = ((part[tid] + part[tid + 64]) + (part[tid + 128] + part[tid + 192])) / (float)p.N;
}

// grid nt (nt + 1) / 2 with nt = ceil(D / 32), block 256
__global__ __launch_bounds__(256) void act_cov_kernel(StatArgs p) {
  __shared__ float xi[kStatStage * kStatLd];
  __shared__ float xj[kStatStage * kStatLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int col = lane & 15, grp = lane >> 4;
  const int wi = wave >> 1, wj = wave & 1;
  const int nt = (p.D + 31) / 32;
  int t = blockIdx.x, ti = 0;
  while (t >= nt - ti) { t -= nt - ti; ++ti; }          // upper tiles row by row: (0, 0 .. nt - 1), (1, 1 .. nt - 1), ...
  const int tj = ti + t;
  // staging: 256 threads cover 4 rows x 64 columns (32 of the i tile, 32 of the j tile) per pass, so a thread's column is fixed
  const int sc = tid & 63, sr = tid >> 6;
  const int gc = (sc < 32 ? ti * 32 : tj * 32) + (sc & 31);
  const float mu = gc < p.D ? p.mean[gc] : 0.f;
  float* sdst = (sc < 32 ? xi : xj) + (sc & 31);
  const float* ai = xi + grp * kStatLd + wi * 16 + col;
  const float* bj = xj + grp * kStatLd + wj * 16 + col;
  f32x4 tot = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < p.N; n0 += kStatChunk) {
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nend = n0 + kStatChunk < p.N ? n0 + kStatChunk : p.N;
    for (int s0 = n0; s0 < nend; s0 += kStatStage) {
      __syncthreads();
      for (int r = sr; r < kStatStage; r += 4) {
        const int n = s0 + r;
        sdst[r * kStatLd] = (n < nend && gc < p.D) ? p.x[(long long)n * p.D + gc] - mu : 0.f;
      }
      __syncthreads();
      const int rows = nend - s0 < kStatStage ? nend - s0 : kStatStage;
      const int kend = (rows + 7) & ~7;                 // (uniform; rows behind nend are zeros)
      for (int k = 0; k < kend; k += 8) {
        a0 = mfma_f32_16x16x4(ai[k * kStatLd], bj[k * kStatLd], a0);
        a1 = mfma_f32_16x16x4(ai[(k + 4) * kStatLd], bj[(k + 4) * kStatLd], a1);
      }
    }
    tot += a0 + a1;
  }
  const float den = (float)(p.N - 1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ti * 32 + wi * 16 + grp * 4 + r, j = tj * 32 + wj * 16 + col;
    if (i <= j && j < p.D) {
      const float v = tot[r] / den;
      p.cov[(long long)i * p.D + j] = v;
      p.cov[(long long)j * p.D + i] = v;
    }
  }
}

struct PairArgs {
  const float* x;      // [N][D]
  const int* ab;       // a [P] | b [P]
  float* out;          // [P]
  int D, P;
};

// grid ceil(P / 4), block 256: one wave per pair
__global__ __launch_bounds__(256) void pair_dist_kernel(PairArgs p) {
  const int lane = threadIdx.x & 63, pair = wave_uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (pair >= p.P) return;
  const float* xa = p.x + (long long)p.ab[pair] * p.D;
  const float* xb = p.x + (long long)p.ab[p.P + pair] * p.D;
  float s = 0.f;
  for (int d = lane; d < p.D; d += 64) {
    const float v = xa[d] - xb[d];
    s = fmaf(v, v, s);
  }
  s = sum64(s);
  if (lane == 0) p.out[pair] = sqrtf(s);
}

}  // namespace mld
