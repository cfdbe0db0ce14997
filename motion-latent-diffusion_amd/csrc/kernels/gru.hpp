// The T2M evaluator towers' own kernels (engine/path_eval.hpp; mldhip_t2m_motion_embed / mldhip_t2m_text_embed): the bidirectional GRU's
// recurrence step and the small elementwise stages around the towers' GEMMs (which run on gemm.hpp's staged tile, EPI = 2).
//
// Replaces: MovementConvEncoder / MotionEncoderBiGRUCo / TextEncoderBiGRUCo (mld/models/architectures/t2m_textenc.py, t2m_motionenc.py) as MLD.t2m_eval
// runs them (mld/models/modeltype/mld.py:618-708), nn.GRU + pack_padded_sequence included.
//
// The recurrence: ONE launch per time step s, both directions and every motion of the call in it.  A workgroup owns 16 hidden units j of one direction
// and the three weight rows j, H + j, 2H + j (r | z | n, PyTorch's gate order) of each, so the three gate products of a unit meet in one lane's
// accumulators; each of its four waves owns 16 motions.  h_prev . W_hh^T runs on MFMAs (exact fp32: v_mfma_f32_16x16x4_f32; split-f16: hi + lo halves,
// three v_mfma_f32_16x16x32_f16 per product, W_hh read from the pre-split image of the weight arena, h split in registers); the gate math, the
// per-motion step mask and the state update follow in the same kernel.  A step reads ALL of h_prev and writes a slice of h_next: the state is double
// buffered by the caller, and a motion that is not active at step s (s >= its length) has its state carried into the other buffer.
// Packed-sequence semantics: the forward direction consumes input row s, the backward direction row len - 1 - s, both for s < len.
// No workgroup waits on another one: the order between steps is the stream's.
#pragma once
#include "rt.hpp"

namespace mld {

constexpr float kLeakySlope = 0.2f;
__device__ __forceinline__ float leaky_relu02(float x) { return x > 0.f ? x : kLeakySlope * x; }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

struct GruStepArgs {
  const float* Whh[2];      // weight_hh_l0 / weight_hh_l0_reverse [3H][H]: the fp32 arena (PREC_F32) or its pre-split image (PREC_F16X3)
  const float* bhh[2];      // bias_hh_l0 / _reverse [3H]: only the n third is read here (b_hr, b_hz are folded into Gi's bias)
  const float* Gi;          // [B x R][6H]: x W_ih^T + b_ih (+ b_hr | b_hz) per (motion, input row); direction-major, then r | z | n
  const float* h_prev;      // [B][2H]: forward state | backward state
  float* h_next;            // the other buffer
  const int* lens;          // [B] steps of each motion (>= 1)
  int B, R, s;              // motions, input rows per motion in Gi, step index
};

// grid (H / 16, ceil(B / 64), 2), block 256
template <int H, int PREC>
__global__ __launch_bounds__(256) void gru_step_kernel(GruStepArgs p) {
  static_assert(H % 128 == 0, "the K loop runs in rounds of four 32-wide chunks");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * 16, d = blockIdx.z;
  const int m0 = blockIdx.y * 64 + wave * 16;
  if (m0 >= p.B) return;                                   // (wave-uniform; the kernel has no barrier)
  const int arow = m0 + r < p.B ? m0 + r : p.B - 1;        // rows behind the last motion: clamped loads, no stores
  const float* hp = p.h_prev + (long long)arow * 2 * H + d * H;
  const float* W = p.Whh[d];
  const float* w0 = W + (long long)(j0 + r) * H;
  const float* w1 = W + (long long)(H + j0 + r) * H;
  const float* w2 = W + (long long)(2 * H + j0 + r) * H;
  // four accumulator sets per gate, one per chunk of a round, summed pairwise at the end: four k-ordered chains of H / 4 instead of one of H (the state feeds itself
  // for up to 49 steps: the shorter chains keep the recurrence within a few float32-CPU errors of float64)
  f32x4 accs[4][3];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int q = 0; q < 3; ++q) accs[x][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kr = 0; kr < H; kr += 128) {
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int k0 = kr + 32 * x;
    f32x4 (&acc)[3] = accs[x];
    const F4 a0 = ld4(hp + k0 + 8 * g), a1 = ld4(hp + k0 + 8 * g + 4);
    if constexpr (PREC == PREC_F32) {
      const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float* wr[3] = {w0, w1, w2};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const F4 b0 = ld4(wr[q] + k0 + 8 * g), b1 = ld4(wr[q] + k0 + 8 * g + 4);
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[q] = mfma_f32_16x16x4(av[i], bv[i], acc[q]);
      }
    } else {
      // the state is produced by this kernel (|h| <= 1 behind the first step; the learned initial state is a weight): split without a clamp
      U4 ahi, alo;
      split16_two(a0.x, a0.y, ahi.x, alo.x);
      split16_two(a0.z, a0.w, ahi.y, alo.y);
      split16_two(a1.x, a1.y, ahi.z, alo.z);
      split16_two(a1.z, a1.w, ahi.w, alo.w);
      const float* wr[3] = {w0, w1, w2};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        // the image of a 32-float group: 16 words of high halves, 16 words of low halves (elementwise.hpp split_bf16_weights_kernel)
        const U4* grp = reinterpret_cast<const U4*>(wr[q] + k0);
        const U4 bhi = grp[g], blo = grp[4 + g];
        acc[q] = mfma_x3_16x16x32(alo, bhi, acc[q]);
        acc[q] = mfma_x3_16x16x32(ahi, blo, acc[q]);
        acc[q] = mfma_x3_16x16x32(ahi, bhi, acc[q]);
      }
    }
  }
  }
  f32x4 acc[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) acc[q] = (accs[0][q] + accs[1][q]) + (accs[2][q] + accs[3][q]);
  const int j = j0 + r;
  const float bn = p.bhh[d][2 * H + j];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + g * 4 + i;
    if (row >= p.B) continue;
    const int len = p.lens[row];
    const float hprev = p.h_prev[(long long)row * 2 * H + d * H + j];
    float hn = hprev;                                     // not active at this step: the state is carried into the other buffer
    if (p.s < len) {
      const int t = d ? len - 1 - p.s : p.s;
      const float* gi = p.Gi + ((long long)row * p.R + t) * (6 * H) + d * 3 * H + j;
      const float rg = sigmoid_f(gi[0] + acc[0][i]);
      const float zg = sigmoid_f(gi[H] + acc[1][i]);
      const float ng = tanhf(gi[2 * H] + rg * (acc[2][i] + bn));
      hn = (1.0f - zg) * ng + zg * hprev;
    }
    p.h_next[(long long)row * 2 * H + d * H + j] = hn;
  }
}

// h[b][d H + j] = hidden[d][j]: the learned initial state of both directions, broadcast over the motions.  grid-stride over B x 2H
__global__ __launch_bounds__(256) void gru_init_kernel(float* __restrict__ h, const float* __restrict__ hidden, int B, int H2) {
  const long long n = (long long)B * H2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) h[i] = hidden[i % H2];
}

// bias of the input-side GRU GEMM, both directions: b_ih + (b_hr | b_hz | 0) -- b_hn stays with the recurrence (it sits inside the r product)
__global__ __launch_bounds__(256) void gru_input_bias_kernel(float* __restrict__ out, const float* __restrict__ bih0, const float* __restrict__ bhh0,
                                                             const float* __restrict__ bih1, const float* __restrict__ bhh1, int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * H) return;
  const int d = i / (3 * H), q = i - d * 3 * H;
  const float* bi = d ? bih1 : bih0;
  const float* bh = d ? bhh1 : bhh0;
  out[i] = bi[q] + (q < 2 * H ? bh[q] : 0.f);
}

// Conv1d weight [O][C][4] -> [O][4][CP] (tap-major, channels zero-padded to CP): with activation rows [time][CP] the four taps of a stride-2
// convolution are contiguous, so the convolution is a GEMM with lda = 2 CP, K = 4 CP.  One thread per output element.
__global__ __launch_bounds__(256) void conv_weight_relay_kernel(const float* __restrict__ w, float* __restrict__ out, int O, int C, int CP) {
  const long long n = (long long)O * 4 * CP;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % CP), tap = (int)((i / CP) % 4);
    const long long o = i / (4 * CP);
    out[i] = c < C ? w[(o * C + c) * 4 + tap] : 0.f;
  }
}

// The motion tower's input staging: feats [B][T][NF] -> G [B][TP][CP], row 0 and rows T + 1 .. TP - 1 of every motion zero (the convolution's own
// padding), row 1 + t = columns 0 .. NF - 5 of frame t, renormalised when asked: g = (f std + mean - mean_eval) / std_eval on ALL T frames -- a padded
// frame (0 in f) becomes a non-zero constant, as in the reference; channels NF - 4 .. CP - 1 zero.  One thread per four output channels (CP % 4 == 0).
__global__ __launch_bounds__(256) void eval_stage_motion_kernel(const float* __restrict__ feats, float* __restrict__ G, const float* __restrict__ mean,
                                                                const float* __restrict__ stdv, const float* __restrict__ mean_eval,
                                                                const float* __restrict__ std_eval, int B, int T, int NF, int TP, int CP, int renorm) {
  const int C = NF - 4, V = CP / 4;
  const long long n = (long long)B * TP * V;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i % V);
    const long long row = i / V;
    const int tp = (int)(row % TP);
    const long long b = row / TP;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (tp >= 1 && tp <= T) {
      const float* f = feats + (b * T + (tp - 1)) * NF;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c4 * 4 + q;
        if (c < C) v[q] = renorm ? (f[c] * stdv[c] + mean[c] - mean_eval[c]) / std_eval[c] : f[c];
      }
    }
    st4(G + row * CP + c4 * 4, F4{v[0], v[1], v[2], v[3]});
  }
}

// The text tower's input rows: x[row][c] = word[row][c] + (pos[row] . Wp[c] + bp[c]) for c < 300 (Linear(15 -> 300) + add), 0 up to the GEMM's K = KP
__global__ __launch_bounds__(256) void eval_stage_text_kernel(const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ Wp,
                                                              const float* __restrict__ bp, float* __restrict__ X, int rows, int DW, int DP, int KP) {
  const long long n = (long long)rows * KP;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % KP);
    const long long row = i / KP;
    float v = 0.f;
    if (c < DW) {
      float s = 0.f;
      for (int k = 0; k < DP; ++k) s += pos[row * DP + k] * Wp[c * DP + k];
      v = word[row * DW + c] + (s + bp[c]);
    }
    X[i] = v;
  }
}

// LayerNorm (two-pass, eps 1e-5) + LeakyReLU(0.2) of rows of width W, in place: the towers' output head.  One workgroup per row.
__global__ __launch_bounds__(256) void eval_ln_lrelu_kernel(float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta, int W) {
  __shared__ float red[4];
  float* x = X + (long long)blockIdx.x * W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float s = 0.f;
  for (int c = tid; c < W; c += 256) s += x[c];
  s = sum64(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / float(W);
  __syncthreads();
  float q = 0.f;
  for (int c = tid; c < W; c += 256) { const float dlt = x[c] - mean; q += dlt * dlt; }
  q = sum64(q);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  const float rstd = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / float(W) + kLnEps);
  for (int c = tid; c < W; c += 256) x[c] = leaky_relu02((x[c] - mean) * rstd * gamma[c] + beta[c]);
}

}  // namespace mld
