// The UESTC recognition ST-GCN (engine/path_uestc.hpp; mldhip_uestc_recognize): rot6d motions [B][24][6][T] -> logits [B][NC] and the 256-d features.
//
// Replaces: STGCN (mld/models/architectures/uestc_stgcn.py, layout 'smpl', strategy 'spatial', edge importance on) in eval mode as UESTCMetrics
// (mld/models/metrics/stgcn.py) runs it.  include/mldhip.h has the math; engine/path_uestc.hpp the folds made at finalize and the order of the launches.
//
// LAYOUT.  Activations are rows of channels.  A PADDED buffer holds [n][v][T + 8][C]: four zero rows in front of and behind the T frame rows of every
// (motion, joint) sequence, so the 9-tap temporal convolution of output step o is ONE row of K = 9 C contiguous floats that starts at padded row s o (stride s).
// A COMPACT buffer holds [n][w][T][KP] rows with no padding rows (the operand of the graph GEMM).
//
// KERNELS (all new, gfx950):
//   stgcn_input_kernel   strided gather of x[n][v][c][t], the data_bn affine, and block 0's graph mix (18 columns, K padded to 128) in one pass;
//   stgcn_mix_kernel     z[n][w][t][k C + c] = sum_v A_k[v][w] x[n][v][t][c]: the graph product made FIRST, on the narrow rows (fp32 VALU, exact in both modes);
//                        the 1x1 graph convolution then is one GEMM of K = 3 Cin whose epilogue adds the per-joint bias table and applies BN's ReLU;
//   stgcn_gemm_kernel    the 64 x (64 | 128) staged tile of kernels/gemm.hpp (same LDS images, same fragment reads, exact-fp32 or split-f16 products, four
//                        accumulator chains) with this net's addressing: A rows by (group, row-in-group) so that overlapping convolution rows and the
//                        stride-2 rows need no copy, a bias ROW per joint, an optional residual, ReLU, and stores into the padded layout of the next block;
//                        K is a run-time multiple of 128 (one instantiation per mode and tile width; loads past the last chunk are clamped, never branched around);
//   stgcn_zero_pads_kernel  the zero rows of a padded buffer (once per geometry change, not per block);
//   stgcn_head_kernel    mean over (t, v), fcn, the non-finite count.
// One tile shape at every row count and fixed summation orders everywhere: a motion's outputs do not depend on what else is in the call.
#pragma once
#include "gemm.hpp"

namespace mld {

constexpr int kStgJoints = 24, kStgIn = 6, kStgK = 3, kStgBlocks = 10, kStgFeat = 256, kStgPad = 4, kStgTaps = 9;
constexpr int kStgA = kStgK * kStgJoints * kStgJoints;      // floats of one [3][24][24] graph operand
// block i: 6 -> 64, 64 -> 64 (x3), 64 -> 128 at stride 2, 128 -> 128 (x2), 128 -> 256 at stride 2, 256 -> 256 (x2)
constexpr int uestc_cout(int i) { return i < 4 ? 64 : i < 7 ? 128 : 256; }
constexpr int uestc_cin(int i) { return i == 0 ? kStgIn : uestc_cout(i - 1); }
constexpr int uestc_stride(int i) { return (i == 4 || i == 7) ? 2 : 1; }

// ReLU that keeps NaN, as torch.relu does (fmaxf(NaN, 0) is 0: a NaN motion would come out finite)
__device__ __forceinline__ float stg_relu(float x) { return x < 0.f ? 0.f : x; }

struct StgInputArgs {
  const float* x; long long sn, sv, sc, st;      // element (n, v, c, t) at x[n sn + v sv + c sc + t st]
  const float* scale; const float* offset;       // data_bn folded: [24][6] each
  const float* Am;                               // A * edge_importance[0]: [3][24][24] as [k][v][w]
  float* Z;                                      // compact [B 24 T][128]: columns k 6 + c, the rest zeros
  int B, T;
};

// grid B * T, block 128: one frame of one motion per workgroup
__global__ __launch_bounds__(128) void stgcn_input_kernel(StgInputArgs p) {
  __shared__ float xs[kStgJoints * kStgIn];
  __shared__ float As[kStgA];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / p.T, t = blockIdx.x - n * p.T;
  for (int i = tid; i < kStgJoints * kStgIn; i += 128) {
    const int v = i / kStgIn, c = i - v * kStgIn;
    xs[i] = p.x[n * p.sn + v * p.sv + c * p.sc + t * p.st] * p.scale[i] + p.offset[i];
  }
  for (int i = tid; i < kStgA; i += 128) As[i] = p.Am[i];
  __syncthreads();
  for (int i = tid; i < kStgJoints * 32; i += 128) {
    const int w = i >> 5, q = i & 31;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = q * 4 + j;
      float s = 0.f;
      if (col < kStgK * kStgIn) {
        const int k = col / kStgIn, c = col - k * kStgIn;
        for (int v = 0; v < kStgJoints; ++v) s = fmaf(As[(k * kStgJoints + v) * kStgJoints + w], xs[v * kStgIn + c], s);
      }
      o[j] = s;
    }
    st4(p.Z + (((long long)n * kStgJoints + w) * p.T + t) * 128 + q * 4, F4{o[0], o[1], o[2], o[3]});
  }
}

struct StgMixArgs {
  const float* X;      // padded [B 24][TP][C]
  const float* Am;     // [3][24][24] as [k][v][w]
  float* Z;            // compact [B 24 T][KP], columns k C + c; columns 3 C .. KP - 1 zeros
  int B, T, TP, KP;
};

// grid ceil(B T / FB), block 256, FB = 256 / C frames per workgroup.  Thread = (channel quad q, frame f, joint group wg of 6 output joints); the joint group is
// the wave index, so the graph coefficients are wave-uniform LDS reads.  72 accumulators per lane; every x quad is read once per wave.
template <int C>
__global__ __launch_bounds__(256) void stgcn_mix_kernel(StgMixArgs p) {
  constexpr int Q = C / 4, FB = 64 / Q;
  __shared__ __attribute__((aligned(16))) float As[kStgK * kStgJoints * 32];      // [k][v][wg][8]: 6 coefficients + 2 unused per slot
  const int tid = threadIdx.x;
  for (int i = tid; i < kStgK * kStgJoints * 32; i += 256) {
    const int j = i & 7, wg = (i >> 3) & 3, kv = i >> 5;
    As[i] = j < 6 ? p.Am[kv * kStgJoints + wg * 6 + j] : 0.f;
  }
  __syncthreads();
  const int q = tid % Q, f = (tid / Q) % FB, wg = wave_uniform(tid >> 6);
  const long long frame = (long long)blockIdx.x * FB + f;
  if (frame >= (long long)p.B * p.T) return;
  const int n = (int)(frame / p.T), t = (int)(frame - (long long)n * p.T);
  F4 acc[kStgK][6];
#pragma unroll
  for (int k = 0; k < kStgK; ++k)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[k][j] = F4{0.f, 0.f, 0.f, 0.f};
  const float* xp = p.X + (((long long)n * kStgJoints) * p.TP + kStgPad + t) * C + q * 4;
#pragma unroll 4
  for (int v = 0; v < kStgJoints; ++v) {
    const F4 x = ld4(xp + (long long)v * p.TP * C);
#pragma unroll
    for (int k = 0; k < kStgK; ++k) {
      const float* ap = As + ((k * kStgJoints + v) * 4 + wg) * 8;
      const F4 a0 = ld4(ap), a1 = ld4(ap + 4);
      const float a[6] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        acc[k][j].x = fmaf(a[j], x.x, acc[k][j].x); acc[k][j].y = fmaf(a[j], x.y, acc[k][j].y);
        acc[k][j].z = fmaf(a[j], x.z, acc[k][j].z); acc[k][j].w = fmaf(a[j], x.w, acc[k][j].w);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float* zr = p.Z + (((long long)n * kStgJoints + wg * 6 + j) * p.T + t) * p.KP;
#pragma unroll
    for (int k = 0; k < kStgK; ++k) st4(zr + k * C + q * 4, acc[k][j]);
    for (int col = kStgK * C + q * 4; col < p.KP; col += 4 * Q) st4(zr + col, F4{0.f, 0.f, 0.f, 0.f});
  }
}

// rows 0 .. 3 and 4 + T .. TP - 1 of each of the G sequences, and `slack` rows behind the last one (a K padded past 9 C / C reads up to one row further)
__global__ __launch_bounds__(256) void stgcn_zero_pads_kernel(float* __restrict__ buf, int G, int T, int TP, int C, int slack) {
  const int cq = C / 4;
  const long long per = (long long)2 * kStgPad * cq, n = (long long)G * per + (long long)slack * cq;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    long long row;
    const int c4 = (int)(i % cq);
    if (i < (long long)G * per) {
      const long long g = i / per;
      const int r = (int)((i - g * per) / cq);
      row = g * TP + (r < kStgPad ? r : T + r);
    } else {
      row = (long long)G * TP + (i - (long long)G * per) / cq;
    }
    st4(buf + row * C + c4 * 4, F4{0.f, 0.f, 0.f, 0.f});
  }
}

struct StgGemmArgs {
  const float* A = nullptr;      // GEMM row m = (group m / rpg, step m % rpg) starts at A + group * a_gs + step * lda
  long long a_gs = 0; int lda = 0; int rpg = 1;
  const float* W = nullptr;      // [N][K]: fp32 (PREC_F32), or the split image of the same table (PREC_F16X3: split at finalize, never in the kernel)
  int K = 0;                     // a multiple of 128
  const float* bias = nullptr;   // [brows][N]: row (group % brows)
  int brows = 1;
  const float* res = nullptr;    // optional, addressed like Y
  float* Y = nullptr;            // row m is stored at row group * y_gr + y_r0 + step, N floats wide
  int y_gr = 1, y_r0 = 0;
  int relu = 0;
  int M = 0, N = 0;
};

// grid (ceil(M / 64), N / (64 NREP)), block 512: 2 x 4 waves, 2 x NREP tiles of 16 x 16 per wave
template <int PREC, int NREP>
__global__ __launch_bounds__(512) void stgcn_gemm_kernel(StgGemmArgs p) {
  static_assert(PREC == PREC_F32 || PREC == PREC_F16X3, "exact fp32 or split-f16");
  constexpr int WM = 2, WN = 4, MREP = 2, BM = WM * MREP * 16, BN = WN * NREP * 16, NT = 512, ROWS = BM + BN, NLD = ROWS * 8 / NT, NLA = BM * 8 / NT;
  static_assert(NLA == 1 && ROWS * 8 % NT == 0, "one A row piece per thread");
  constexpr int CST = BN + 4;
  static_assert(BM * CST <= 2 * ROWS * kGemmLdsStride, "the parked tile fits the chunk buffers");
  __shared__ __attribute__((aligned(16))) float smem[2 * ROWS * kGemmLdsStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  const int bm0 = blockIdx.x * BM, bn0 = blockIdx.y * BN;
  const int KCS = p.K / 32;

  const float* src[NLD];
  {
    const int row = tid >> 3, c4 = tid & 7;
    int m = bm0 + row;
    m = m < p.M ? m : p.M - 1;
    const int grp = m / p.rpg, step = m - grp * p.rpg;
    src[0] = p.A + (long long)grp * p.a_gs + (long long)step * p.lda + c4 * 4;
#pragma unroll
    for (int j = NLA; j < NLD; ++j) {
      const int idx = tid + j * NT, wrow = idx >> 3;
      int n = bn0 + wrow - BM;
      n = n < p.N ? n : p.N - 1;
      src[j] = p.W + (long long)n * p.K + c4 * 4;
    }
  }
  F4 st0[NLD], st1[NLD], st2[NLD], st3[NLD];
  auto gload = [&](F4(&stage)[NLD], int kc) {
    kc = kc < KCS ? kc : KCS - 1;      // behind the last chunk: a valid address, a value nobody multiplies
#pragma unroll
    for (int j = 0; j < NLD; ++j) stage[j] = ld4(src[j] + kc * 32);
  };
  auto lstore = [&](int buf, F4(&stage)[NLD]) {
    float* dst = smem + buf * ROWS * kGemmLdsStride;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = tid + j * NT, row = idx >> 3, c4 = idx & 7;
      const F4 v = stage[j];
      if constexpr (PREC == PREC_F32) {
        st4(dst + row * kGemmLdsStride + c4 * 4, v);
      } else {
        if (j >= NLA) { st4(dst + row * kGemmLdsStride + c4 * 4, v); continue; }      // weight rows: already the row image
        // activation rows are split WITHOUT a range clamp: a NaN stays a NaN (it must reach the outputs of its motion and the non-finite counter), and a value
        // beyond +-65 504 ends as inf / NaN there instead of a saturated, finite, wrong row (mldhip.h "Range contract"; the probe reads such weights and falls back)
        unsigned h0, l0, h1, l1;
        split16_two(v.x, v.y, h0, l0);
        split16_two(v.z, v.w, h1, l1);
        unsigned* rowp = reinterpret_cast<unsigned*>(dst + row * kGemmLdsStride);
        *reinterpret_cast<uint2_t*>(rowp + c4 * 2) = uint2_t{h0, h1};
        *reinterpret_cast<uint2_t*>(rowp + 16 + c4 * 2) = uint2_t{l0, l1};
      }
    }
  };
  f32x4 acc[4][MREP][NREP];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int a = 0; a < MREP; ++a)
#pragma unroll
      for (int b = 0; b < NREP; ++b) acc[x][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&](int buf, f32x4 (&dst)[MREP][NREP]) {
    const float* as = smem + buf * ROWS * kGemmLdsStride + (wm * MREP * 16 + r) * kGemmLdsStride;
    const float* ws = smem + buf * ROWS * kGemmLdsStride + (BM + wn * NREP * 16 + r) * kGemmLdsStride;
    if constexpr (PREC == PREC_F32) {
      Frag fa[MREP], fb[NREP];
#pragma unroll
      for (int t = 0; t < MREP; ++t) {
        const F4 a = ld4(as + t * 16 * kGemmLdsStride + g * 4), b = ld4(as + t * 16 * kGemmLdsStride + g * 4 + 16);
        fa[t].v[0] = a.x; fa[t].v[1] = a.y; fa[t].v[2] = a.z; fa[t].v[3] = a.w;
        fa[t].v[4] = b.x; fa[t].v[5] = b.y; fa[t].v[6] = b.z; fa[t].v[7] = b.w;
      }
#pragma unroll
      for (int t = 0; t < NREP; ++t) {
        const F4 a = ld4(ws + t * 16 * kGemmLdsStride + g * 4), b = ld4(ws + t * 16 * kGemmLdsStride + g * 4 + 16);
        fb[t].v[0] = a.x; fb[t].v[1] = a.y; fb[t].v[2] = a.z; fb[t].v[3] = a.w;
        fb[t].v[4] = b.x; fb[t].v[5] = b.y; fb[t].v[6] = b.z; fb[t].v[7] = b.w;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int a = 0; a < MREP; ++a)
#pragma unroll
          for (int b = 0; b < NREP; ++b) dst[a][b] = mfma_f32_16x16x4(fa[a].v[i], fb[b].v[i], dst[a][b]);
    } else {
      U4 ahi[MREP], alo[MREP], bhi[NREP], blo[NREP];
#pragma unroll
      for (int t = 0; t < MREP; ++t) {
        const U4* rp = reinterpret_cast<const U4*>(as + t * 16 * kGemmLdsStride);
        ahi[t] = rp[g];
        alo[t] = rp[4 + g];
      }
#pragma unroll
      for (int t = 0; t < NREP; ++t) {
        const U4* rp = reinterpret_cast<const U4*>(ws + t * 16 * kGemmLdsStride);
        bhi[t] = rp[g];
        blo[t] = rp[4 + g];
      }
#pragma unroll
      for (int a = 0; a < MREP; ++a)
#pragma unroll
        for (int b = 0; b < NREP; ++b) {
          dst[a][b] = mfma_x3_16x16x32(alo[a], bhi[b], dst[a][b]);
          dst[a][b] = mfma_x3_16x16x32(ahi[a], blo[b], dst[a][b]);
          dst[a][b] = mfma_x3_16x16x32(ahi[a], bhi[b], dst[a][b]);
        }
    }
  };
  // the chunk pipeline of kernels/gemm.hpp (4-deep register ring, LDS double buffer, one barrier per chunk), as a run-time loop over rounds of four chunks
  gload(st0, 0);
  gload(st1, 1);
  gload(st2, 2);
  gload(st3, 3);
  lstore(0, st0);
  gload(st0, 4);
  __syncthreads();
  for (int kc = 0; kc < KCS; kc += 4) {
    mma(0, acc[0]);
    lstore(1, st1);
    gload(st1, kc + 5);
    __syncthreads();
    mma(1, acc[1]);
    lstore(0, st2);
    gload(st2, kc + 6);
    __syncthreads();
    mma(0, acc[2]);
    lstore(1, st3);
    gload(st3, kc + 7);
    __syncthreads();
    mma(1, acc[3]);
    lstore(0, st0);
    gload(st0, kc + 8);
    __syncthreads();
  }
  // park the raw sums; bias row, residual, ReLU and the row mapping happen on the way out, in 16-byte pieces
  float* Cs = smem;
#pragma unroll
  for (int a = 0; a < MREP; ++a)
#pragma unroll
    for (int b = 0; b < NREP; ++b) {
      const f32x4 s = (acc[0][a][b] + acc[1][a][b]) + (acc[2][a][b] + acc[3][a][b]);
#pragma unroll
      for (int i = 0; i < 4; ++i) Cs[(wm * MREP * 16 + a * 16 + g * 4 + i) * CST + wn * NREP * 16 + b * 16 + r] = s[i];
    }
  __syncthreads();
  constexpr int V = BN / 4;
#pragma unroll
  for (int j = 0; j < BM * V / NT; ++j) {
    const int idx = tid + j * NT, row = idx / V, c4 = idx - row * V;
    const int m = bm0 + row, col = bn0 + c4 * 4;
    if (m < p.M && col < p.N) {
      const int grp = m / p.rpg, step = m - grp * p.rpg;
      const long long orow = (long long)grp * p.y_gr + p.y_r0 + step;
      F4 v = ld4(Cs + row * CST + c4 * 4);
      const F4 bq = ld4(p.bias + (long long)(grp % p.brows) * p.N + col);
      v = F4{v.x + bq.x, v.y + bq.y, v.z + bq.z, v.w + bq.w};
      if (p.res) {
        const F4 x = ld4(p.res + orow * p.N + col);
        v = F4{v.x + x.x, v.y + x.y, v.z + x.z, v.w + x.w};
      }
      if (p.relu) v = F4{stg_relu(v.x), stg_relu(v.y), stg_relu(v.z), stg_relu(v.w)};
      st4(p.Y + orow * p.N + col, v);
    }
  }
}

struct StgHeadArgs {
  const float* X;        // padded [B 24][TP][256]: the last block's output
  const float* fw; const float* fb;      // fcn [NC][256], [NC]
  float* logits;         // [B][NC] or NULL
  float* feat;           // [B][256] or NULL
  unsigned* counter;     // non-finite outputs (NULL: not counted)
  int T, TP, NC;
};

// grid B, block 256: thread c sums channel c over (v, t) in a fixed order (four chains over t), then thread j < NC makes logit j
__global__ __launch_bounds__(256) void stgcn_head_kernel(StgHeadArgs p) {
  __shared__ float fs[kStgFeat];
  const int c = threadIdx.x, n = blockIdx.x;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int v = 0; v < kStgJoints; ++v) {
    const float* xp = p.X + (((long long)n * kStgJoints + v) * p.TP + kStgPad) * kStgFeat + c;
    for (int t = 0; t < p.T; ++t) s[t & 3] += xp[(long long)t * kStgFeat];
  }
  const float f = ((s[0] + s[1]) + (s[2] + s[3])) / (float)(kStgJoints * p.T);
  fs[c] = f;
  float bad = 0.f;
  if (p.feat) { p.feat[(long long)n * kStgFeat + c] = f; bad += nonfinite_f(f); }
  __syncthreads();
  if (p.logits && c < p.NC) {
    const float* w = p.fw + (long long)c * kStgFeat;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < kStgFeat; k += 4) {
      const F4 wq = ld4(w + k);
      a[0] = fmaf(fs[k], wq.x, a[0]); a[1] = fmaf(fs[k + 1], wq.y, a[1]); a[2] = fmaf(fs[k + 2], wq.z, a[2]); a[3] = fmaf(fs[k + 3], wq.w, a[3]);
    }
    const float y = ((a[0] + a[1]) + (a[2] + a[3])) + p.fb[c];
    p.logits[(long long)n * p.NC + c] = y;
    bad += nonfinite_f(y);
  }
  if (p.counter) add_count(p.counter, bad);
}

}  // namespace mld
