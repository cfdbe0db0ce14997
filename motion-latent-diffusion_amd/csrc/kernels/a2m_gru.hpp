// The HumanAct12 action-recognition GRU (engine/path_a2m.hpp; mldhip_a2m_recognize): joints [B][T][72] -> logits [B][12] and the 30-d activations the
// FID is computed from.
//
// Replaces: MotionDiscriminator / MotionDiscriminatorForFID (mld/models/architectures/humanact12_gru.py) as HUMANACTMetrics runs them
// (mld/models/metrics/gru.py): nn.GRU(72, 128, 2 layers) over the padded sequence, the top layer's output at step len - 1, Linear(128 -> 30), tanh,
// Linear(30 -> 12).  include/mldhip.h has the math, the padded-frame rule and the h0 contract.
//
// ONE launch per call.  A workgroup owns a MOTION TILE of 16 motions (the row count of v_mfma_f32_16x16x4_f32) and runs both layers over all of the
// tile's steps, then the head; no workgroup waits on another.  Eight waves; wave w owns hidden units 16 w .. 16 w + 15 of BOTH layers and the three
// gate columns r | z | n (PyTorch's order) of each, so the gate products of a unit meet in one lane's accumulators (D row = motion, D column = unit).
// The layers run as a two-stage pipeline: phase p computes layer 0 at step p and layer 1 at step p - 1; both read h0 after step p - 1 (the recurrent
// operand of layer 0 and the input operand of layer 1 are the same A values), so a phase needs ONE barrier.  The state of both layers lives in LDS,
// double buffered per layer; x_t is prefetched into registers one phase ahead.  A motion is updated at step s only while s < len (its state is carried
// past len, so the final state is its step len - 1 output) and its frames t >= len are never read.  The tile runs max(len) + 1 phases.
// K order: lane group g (lane >> 4) of MFMA i in a 32-wide chunk takes k = k0 + 8 g + i (the A and B operands agree, so the products are the same sums;
// a lane loads 8 consecutive k of its row with two 16-byte loads).  Two accumulator chains per (gate, operand) -- even and odd i -- added at the end.
// The head (linear1 + tanh on 480 lanes, then linear2 on 192) is fp32 VALU on the tile's final states in LDS.
// Exact fp32 in every precision mode (no split-f16 form, no stage of the range contract): the arithmetic does not depend on the handle's mode.
//
// PRICE (an ESTIMATE, written before the kernel was built; profiles/a2m_rec_ab.json has what was measured):
//   MFMAs per phase per tile: 8 unit slices x 3 gates x (18 [x W_ih0, K 72] + 32 [h0 W_hh0] + 32 [h0 W_ih1] + 32 [h1 W_hh1]) = 2 736, i.e. 684 per
//   SIMD x 32 issue cycles = 21.9 k cycles = 9.1 us at 2.4 GHz -- the floor of a phase on one CU (the MFMA pipe; 342 per wave, 24 independent chains).
//   Weight bytes per phase per tile: 3 x 384 x 128 x 4 + 384 x 72 x 4 = 700 KB, streamed from L2 (the 700 KB of weights do not fit in LDS (160 KB) or
//   in the waves' registers (96 floats per lane per matrix slice); they are L2-resident and shared by every tile): about 11 k cycles at 64 B / clk / CU,
//   under the MFMA floor when two waves per SIMD overlap each other's loads with their products.  State traffic is LDS only (2 x 8 KB per phase).
//   A call of T = 60 frames: 61 phases x ~9 us = ~0.56 ms at any B up to 16 x 256 (one tile per CU); the head adds ~1 us.
#pragma once
#include "rt.hpp"

namespace mld {

constexpr int kA2mIn = 72, kA2mH = 128, kA2mG = 3 * kA2mH, kA2mL1 = 30, kA2mCls = 12, kA2mTile = 16;
constexpr int kA2mHP = kA2mH + 4;       // LDS row stride of the states: 16 rows x 16-byte reads land on distinct banks
constexpr int kA2mXK = kA2mIn / 4;      // x W_ih0: the whole K = 72 is one chunk, 18 k per lane group

struct A2mArgs {
  const float* x;                       // [B][T][72] joints, feature 3 joint + coord
  const int* lens;                      // [B] steps of each motion (1 .. T)
  const float* h0;                      // [2][B][128] initial state of both layers, or NULL (zeros)
  const float *wih0, *whh0, *wih1, *whh1;   // [384][72], [384][128] x 3 (recurrent.weight_*)
  const float *bih0, *bhh0, *bih1, *bhh1;   // [384] each
  const float *w1, *b1, *w2, *b2;           // linear1 [30][128] + [30], linear2 [12][30] + [12]
  float* logits;                        // [B][12] or NULL
  float* act;                           // [B][30] or NULL
  unsigned* counter;                    // non-finite outputs
  int B, T;
};

// (sigmoid_f, nonfinite_f and add_count come from gru.hpp / smpl.hpp of the same translation unit)

// grid ceil(B / 16), block 512
__global__ __launch_bounds__(512) void a2m_gru_kernel(A2mArgs p) {
  __shared__ __attribute__((aligned(16))) float hs[2][2][kA2mTile * kA2mHP];   // [layer][buffer][motion][unit]
  __shared__ float act_s[kA2mTile * 32];
  __shared__ int lens_s[kA2mTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int col = lane & 15, grp = lane >> 4;
  const int b0 = blockIdx.x * kA2mTile;
  if (tid < kA2mTile) lens_s[tid] = b0 + tid < p.B ? p.lens[b0 + tid] : 0;
  // initial states: h0[layer][b] for the tile's motions, zeros for NULL and for rows behind the last motion
  for (int i = tid; i < 2 * kA2mTile * kA2mH; i += 512) {
    const int l = i / (kA2mTile * kA2mH), m = (i / kA2mH) % kA2mTile, k = i % kA2mH;
    const int b = b0 + m;
    hs[l][0][m * kA2mHP + k] = (p.h0 && b < p.B) ? p.h0[((long long)l * p.B + b) * kA2mH + k] : 0.f;
  }
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int m = 0; m < kA2mTile; ++m) tmax = lens_s[m] > tmax ? lens_s[m] : tmax;
  tmax = wave_uniform(tmax);

  const int j = wave * 16 + col;                 // this lane's unit: B-operand column and D column
  float bi0[3], bh0[3], bi1[3], bh1[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) { bi0[q] = p.bih0[q * kA2mH + j]; bh0[q] = p.bhh0[q * kA2mH + j]; bi1[q] = p.bih1[q * kA2mH + j]; bh1[q] = p.bhh1[q * kA2mH + j]; }
  // the A-operand row of this lane (motion col of the tile): x of step t is read only for t < len
  const int alen = lens_s[col];
  const float* xrow = p.x + ((long long)(b0 + col) * p.T) * kA2mIn + kA2mXK * grp;
  float xa[kA2mXK];
#pragma unroll
  for (int i = 0; i < kA2mXK; ++i) xa[i] = 0 < alen ? xrow[i] : 0.f;

  for (int ph = 0; ph <= tmax; ++ph) {
    const bool do0 = ph < tmax, do1 = ph >= 1;     // (uniform)
    const float* h0in = hs[0][ph & 1];               // layer 0 after step ph - 1
    const float* h1in = hs[1][(ph + 1) & 1];         // layer 1 after step ph - 2
    f32x4 gi0[3][2], gh0[3][2], gi1[3][2], gh1[3][2];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int c = 0; c < 2; ++c) gi0[q][c] = gh0[q][c] = gi1[q][c] = gh1[q][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (do0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float* w = p.wih0 + (long long)(q * kA2mH + j) * kA2mIn + kA2mXK * grp;
        float bv[kA2mXK];
#pragma unroll
        for (int i = 0; i < kA2mXK; ++i) bv[i] = w[i];
#pragma unroll
        for (int i = 0; i < kA2mXK; ++i) gi0[q][i & 1] = mfma_f32_16x16x4(xa[i], bv[i], gi0[q][i & 1]);
      }
    }
    // prefetch x of the next step (consumed by the next phase's layer 0)
    {
      const int tn = ph + 1;
      const float* xs = xrow + (long long)tn * kA2mIn;
#pragma unroll
      for (int i = 0; i < kA2mXK; ++i) xa[i] = tn < alen ? xs[i] : 0.f;
    }
#pragma unroll
    for (int kc = 0; kc < kA2mH; kc += 32) {
      const F4 a0l = ld4(h0in + col * kA2mHP + kc + 8 * grp), a0h = ld4(h0in + col * kA2mHP + kc + 8 * grp + 4);
      const float a0[8] = {a0l.x, a0l.y, a0l.z, a0l.w, a0h.x, a0h.y, a0h.z, a0h.w};
      if (do0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float* w = p.whh0 + (long long)(q * kA2mH + j) * kA2mH + kc + 8 * grp;
          const F4 bl = ld4(w), bh = ld4(w + 4);
          const float bv[8] = {bl.x, bl.y, bl.z, bl.w, bh.x, bh.y, bh.z, bh.w};
#pragma unroll
          for (int i = 0; i < 8; ++i) gh0[q][i & 1] = mfma_f32_16x16x4(a0[i], bv[i], gh0[q][i & 1]);
        }
      }
      if (do1) {
        const F4 a1l = ld4(h1in + col * kA2mHP + kc + 8 * grp), a1h = ld4(h1in + col * kA2mHP + kc + 8 * grp + 4);
        const float a1[8] = {a1l.x, a1l.y, a1l.z, a1l.w, a1h.x, a1h.y, a1h.z, a1h.w};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float* wi = p.wih1 + (long long)(q * kA2mH + j) * kA2mH + kc + 8 * grp;
          const float* wh = p.whh1 + (long long)(q * kA2mH + j) * kA2mH + kc + 8 * grp;
          const F4 il = ld4(wi), ih = ld4(wi + 4), hl = ld4(wh), hh = ld4(wh + 4);
          const float bvi[8] = {il.x, il.y, il.z, il.w, ih.x, ih.y, ih.z, ih.w};
          const float bvh[8] = {hl.x, hl.y, hl.z, hl.w, hh.x, hh.y, hh.z, hh.w};
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            gi1[q][i & 1] = mfma_f32_16x16x4(a0[i], bvi[i], gi1[q][i & 1]);
            gh1[q][i & 1] = mfma_f32_16x16x4(a1[i], bvh[i], gh1[q][i & 1]);
          }
        }
      }
      sched_fence();
    }
    // gate math and state update of this lane's (motion, unit) cells: D row grp 4 + r, column j
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = grp * 4 + r, len = lens_s[m];
      if (do0) {
        const float hp = h0in[m * kA2mHP + j];
        float hn = hp;                                   // step ph >= len: carried
        if (ph < len) {
          const float rg = sigmoid_f(((gi0[0][0][r] + gi0[0][1][r]) + bi0[0]) + ((gh0[0][0][r] + gh0[0][1][r]) + bh0[0]));
          const float zg = sigmoid_f(((gi0[1][0][r] + gi0[1][1][r]) + bi0[1]) + ((gh0[1][0][r] + gh0[1][1][r]) + bh0[1]));
          const float ng = tanhf(((gi0[2][0][r] + gi0[2][1][r]) + bi0[2]) + rg * ((gh0[2][0][r] + gh0[2][1][r]) + bh0[2]));
          hn = (hp - ng) * zg + ng;
        }
        hs[0][(ph + 1) & 1][m * kA2mHP + j] = hn;
      }
      if (do1) {
        const float hp = h1in[m * kA2mHP + j];
        float hn = hp;
        if (ph - 1 < len) {
          const float rg = sigmoid_f(((gi1[0][0][r] + gi1[0][1][r]) + bi1[0]) + ((gh1[0][0][r] + gh1[0][1][r]) + bh1[0]));
          const float zg = sigmoid_f(((gi1[1][0][r] + gi1[1][1][r]) + bi1[1]) + ((gh1[1][0][r] + gh1[1][1][r]) + bh1[1]));
          const float ng = tanhf(((gi1[2][0][r] + gi1[2][1][r]) + bi1[2]) + rg * ((gh1[2][0][r] + gh1[2][1][r]) + bh1[2]));
          hn = (hp - ng) * zg + ng;
        }
        hs[1][ph & 1][m * kA2mHP + j] = hn;
      }
    }
    __syncthreads();
  }

  // head: the top layer's state after step len - 1 of each motion is in hs[1][tmax & 1]
  const float* hf = hs[1][tmax & 1];
  float bad = 0.f;
  if (tid < kA2mTile * kA2mL1) {
    const int m = tid / kA2mL1, o = tid % kA2mL1;
    const float* w = p.w1 + o * kA2mH;
    const float* h = hf + m * kA2mHP;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int k = 0; k < kA2mH; k += 4)
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = fmaf(h[k + c], w[k + c], s[c]);
    const float a = tanhf(((s[0] + s[1]) + (s[2] + s[3])) + p.b1[o]);
    act_s[m * 32 + o] = a;
    if (p.act && b0 + m < p.B) {
      bad += nonfinite_f(a);
      p.act[(long long)(b0 + m) * kA2mL1 + o] = a;
    }
  }
  __syncthreads();
  if (p.logits && tid < kA2mTile * kA2mCls) {
    const int m = tid / kA2mCls, o = tid % kA2mCls;
    const float* w = p.w2 + o * kA2mL1;
    const float* a = act_s + m * 32;
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kA2mL1; k += 2) { s[0] = fmaf(a[k], w[k], s[0]); s[1] = fmaf(a[k + 1], w[k + 1], s[1]); }
    const float v = (s[0] + s[1]) + p.b2[o];
    if (b0 + m < p.B) {
      bad += nonfinite_f(v);
      p.logits[(long long)(b0 + m) * kA2mCls + o] = v;
    }
  }
  add_count(p.counter, bad);
}

}  // namespace mld
