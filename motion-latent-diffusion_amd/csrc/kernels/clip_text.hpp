// CLIP text tower (transformers CLIPTextTransformer + text_projection) on RAGGED rows: prompt p contributes the n_p = eos_pos[p] + 1
// token rows up to and including its EOS token -- the attention is causal and the output is read at the EOS row, so no later row can
// reach it -- packed back to back into one [sum n_p][D] activation.  Replaces the text branch of mld/models/architectures/mld_clip.py:53-78
// (tokenizer output -> get_text_features).  The GEMMs run on gemm.hpp's staged tile (EPI = 1: quick-GELU / plain residual epilogues);
// this file holds what is not a GEMM: the embedding gather, the width-D LayerNorm (optionally through a row gather: the EOS rows in
// front of final_layer_norm), the causal self-attention and the scatter of the unique prompts' embeddings to every duplicate.
#pragma once
#include "attention.hpp"
#include "rt.hpp"

namespace mld {

constexpr int kClipKeyTiles = 5;                    // 16-key tiles per prompt: clip_ctx <= 80
constexpr int kClipAttnWaves = 4;
constexpr int kClipAttnLdsBytes = 2 * kClipKeyTiles * 16 * 68 * 4;      // fp32 K and V of one (prompt, head), row stride 68 (attn_decode_kernel's layout)

// X[row] = token_embedding[row_tok[row]] + position_embedding[row_pos[row]]; 16-byte loads and stores
__global__ __launch_bounds__(256) void clip_embed_kernel(const float* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                                         const int* __restrict__ row_tok, const int* __restrict__ row_pos,
                                                         float* __restrict__ X, int rows, int D) {
  const int V = D / 4;
  const long long n4 = (long long)rows * V;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const int row = (int)(i / V), c4 = (int)(i - (long long)row * V);
    const F4 a = ld4(tok_emb + (long long)row_tok[row] * D + c4 * 4), b = ld4(pos_emb + (long long)row_pos[row] * D + c4 * 4);
    st4(X + (long long)row * D + c4 * 4, F4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w});
  }
}

// LayerNorm over rows of width 256 NV (two-pass, like ATen's): one wave per row, 4 rows per workgroup.  `gather` != nullptr: output row
// m normalises input row gather[m] (the EOS rows in front of final_layer_norm).
template <int NV>
__global__ __launch_bounds__(256) void clip_layernorm_kernel(const float* __restrict__ X, float* __restrict__ Y, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const int* __restrict__ gather, int M) {
  constexpr int D = 256 * NV;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int row = blockIdx.x * 4 + wave;
  const bool live = row < M;
  row = live ? row : M - 1;
  const long long src = gather ? gather[row] : row;
  F4 x[NV];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    x[j] = ld4(X + src * D + j * 256 + lane * 4);
    s += (x[j].x + x[j].y) + (x[j].z + x[j].w);
  }
  const float mean = sum64(s) * (1.0f / float(D));
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    x[j].x -= mean; x[j].y -= mean; x[j].z -= mean; x[j].w -= mean;
    q += (x[j].x * x[j].x + x[j].y * x[j].y) + (x[j].z * x[j].z + x[j].w * x[j].w);
  }
  const float rs = rsqrtf(sum64(q) * (1.0f / float(D)) + kLnEps);
  if (!live) return;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const F4 gm = ld4(gamma + j * 256 + lane * 4), bt = ld4(beta + j * 256 + lane * 4);
    st4(Y + (long long)row * D + j * 256 + lane * 4, F4{x[j].x * rs * gm.x + bt.x, x[j].y * rs * gm.y + bt.y, x[j].z * rs * gm.z + bt.z, x[j].w * rs * gm.w + bt.w});
  }
}

// out[p] = E[dup[p]]: every prompt of the call reads the embedding of its unique representative
__global__ __launch_bounds__(256) void clip_scatter_kernel(const float* __restrict__ E, const int* __restrict__ dup, float* __restrict__ out, int P, int D) {
  const int V = D / 4;
  const long long n4 = (long long)P * V;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const int p = (int)(i / V), c4 = (int)(i - (long long)p * V);
    st4(out + (long long)p * D + c4 * 4, ld4(E + (long long)dup[p] * D + c4 * 4));
  }
}

// Causal self-attention of the packed rows, exact-fp32 MFMAs: attn_decode_kernel's structure (K and V of one (prompt, head) staged once in
// LDS at row stride 68, S^T = K Q^T so that a lane owns one query column, P feeds P V from its registers) with the rows of prompt p at
// off[p] .. off[p] + n[p] - 1, key j masked for query i when j > i, and key tiles above the query tile's diagonal never multiplied.
// There is no key-padding mask: padding rows do not exist.  qkv [rows][3 D] (q | k | v, heads = 64-column slices), o [rows][D].
__global__ __launch_bounds__(kClipAttnWaves * 64) void clip_attn_kernel(const float* __restrict__ qkv, float* __restrict__ o, const int* __restrict__ off,
                                                                        const int* __restrict__ cnt, int H) {
  constexpr int HD = 64, LDS_STRIDE = 68, NKT = kClipKeyTiles, NW = kClipAttnWaves;
#if defined(MLDHIP_SIM)
  float* smem = reinterpret_cast<float*>(hipsim::blk().dyn_smem.data());
#else
  extern __shared__ __attribute__((aligned(16))) float smem[];
#endif
  const int D = H * HD;
  const int p = blockIdx.x / H, h = blockIdx.x % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int len = cnt[p] < NKT * 16 ? cnt[p] : NKT * 16;
  const long long row0 = off[p];
  const int nkt = (len + 15) >> 4;
  float* Ks = smem;
  float* Vs = smem + (size_t)NKT * 16 * LDS_STRIDE;
  {
    constexpr int KPI = NW * 4, NIT = (NKT * 16 + KPI - 1) / KPI;
    const int c4 = tid & 15, k0 = tid >> 4;
    const float* base = qkv + row0 * 3 * D + h * HD + c4 * 4;
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      float* dst = op == 0 ? Ks : Vs;
      const float* src = base + (op + 1) * D;
      F4 v[NIT];
#pragma unroll
      for (int j = 0; j < NIT; ++j) {
        const int key = j * KPI + k0;
        const int kc = key < len ? key : len - 1;
        v[j] = ld4(src + (long long)kc * 3 * D);
      }
#pragma unroll
      for (int j = 0; j < NIT; ++j) {
        const int key = j * KPI + k0;
        const float m = key < len ? 1.f : 0.f;      // P is 0 there and 0 * garbage must not be NaN
        if (key < nkt * 16) st4(dst + key * LDS_STRIDE + c4 * 4, F4{v[j].x * m, v[j].y * m, v[j].z * m, v[j].w * m});
      }
    }
  }
  __syncthreads();

  for (int qt = wave; qt < nkt; qt += NW) {
    int qrow = qt * 16 + r;
    qrow = qrow < len ? qrow : len - 1;
    const float* qp = qkv + (row0 + qrow) * 3 * D + h * HD + g * 16;
    float qf[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      F4 t = ld4(qp + c * 4);
      qf[c * 4] = t.x * 0.125f; qf[c * 4 + 1] = t.y * 0.125f; qf[c * 4 + 2] = t.z * 0.125f; qf[c * 4 + 3] = t.w * 0.125f;      // head_dim^-0.5, exact
    }
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kt <= qt) {
        const float* kp = Ks + (kt * 16 + r) * LDS_STRIDE + g * 16;
        float kf[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          F4 t = ld4(kp + c * 4);
          kf[c * 4] = t.x; kf[c * 4 + 1] = t.y; kf[c * 4 + 2] = t.z; kf[c * 4 + 3] = t.w;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kt] = mfma_f32_16x16x4(kf[i], qf[i], s[kt]);
      }
    }
    // causal softmax down each query column: this lane holds keys kt*16 + g*4 + i of query qt*16 + r
    const int query = qt * 16 + r;
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt * 16 + g * 4 + i;
        const bool valid = kt <= qt && key < len && (key <= query || query >= len);      // (queries past the last row are never stored: kept finite)
        s[kt][i] = valid ? s[kt][i] : -INFINITY;
        m = fmaxf(m, s[kt][i]);
      }
    m = max_groups(m);
    float den = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float e = expf(s[kt][i] - m);
        s[kt][i] = e;
        den += e;
      }
    den = sum_groups(den);
    const float inv = 1.0f / den;
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt <= qt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pv = s[kt][i] * inv;
          const float* vp = Vs + (kt * 16 + g * 4 + i) * LDS_STRIDE + r;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma_f32_16x16x4(pv, vp[dt * 16], oacc[dt]);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = qt * 16 + g * 4 + i;
        if (q < len) o[(row0 + q) * D + h * HD + dt * 16 + r] = oacc[dt][i];
      }
  }
}

// Split-f16 form (MLDHIP_PREC_F16X3): attn_decode_x3_kernel's operand layouts -- K as two half planes [key][64 dims], V^T as two half
// planes [dim][keys], every product as lo*hi + hi*lo + hi*hi on v_mfma_f32_16x16x32_f16, fp32 softmax in the log2 domain -- with the same
// ragged rows and causal mask as clip_attn_kernel.  P V runs over 32-key blocks: block kb is multiplied when its first tile is on or
// below the query tile's diagonal (the masked scores of its second tile are exact zeros).
__global__ __launch_bounds__(kClipAttnWaves * 64) void clip_attn_x3_kernel(const float* __restrict__ qkv, float* __restrict__ o, const int* __restrict__ off,
                                                                           const int* __restrict__ cnt, int H) {
  constexpr int HD = 64, NKT = kClipKeyTiles, NW = kClipAttnWaves, KST = attn_x3_kstride<NKT>(), VST = attn_x3_vt_stride<NKT>(), NKB = (NKT + 1) / 2;
#if defined(MLDHIP_SIM)
  unsigned* smem = reinterpret_cast<unsigned*>(hipsim::blk().dyn_smem.data());
#else
  extern __shared__ __attribute__((aligned(16))) unsigned smem_u[];
  unsigned* smem = smem_u;
#endif
  unsigned* Kh = smem;                       // [NKT*16][KST]
  unsigned* Kl = Kh + NKT * 16 * KST;
  unsigned* Vh = Kl + NKT * 16 * KST;        // [64][VST]  (V^T: row = head dim, column = key)
  unsigned* Vl = Vh + 64 * VST;
  const int D = H * HD;
  const int p = blockIdx.x / H, h = blockIdx.x % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int len = cnt[p] < NKT * 16 ? cnt[p] : NKT * 16;
  const long long row0 = off[p];
  const int nkt = (len + 15) >> 4, nkb = (nkt + 1) >> 1;
  {
    constexpr int KPI = NW * 4, NIT = (NKB * 32 + KPI - 1) / KPI;
    const int c4 = tid & 15, k0 = tid >> 4;
    const float* base = qkv + row0 * 3 * D + h * HD + c4 * 4;
    F4 v[NIT];
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int key = j * KPI + k0;
      const int kc = key < len ? key : len - 1;
      v[j] = ld4(base + D + (long long)kc * 3 * D);
    }
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int key = j * KPI + k0;
      const float m = key < len ? 1.f : 0.f;
      if (key < nkt * 16) {
        unsigned h0, l0, h1, l1;
        split16_pair(v[j].x * m, v[j].y * m, h0, l0);
        split16_pair(v[j].z * m, v[j].w * m, h1, l1);
        *reinterpret_cast<U2*>(Kh + key * KST + c4 * 2) = U2{h0, h1};
        *reinterpret_cast<U2*>(Kl + key * KST + c4 * 2) = U2{l0, l1};
      }
    }
    // V^T: a thread owns one head dim and four consecutive keys (attn_decode_x3_kernel: one 8-byte LDS store per plane)
    constexpr int NVG = NKB * 8, NVI = (NVG + NW - 1) / NW;
    const int vd = tid & 63, vg0 = tid >> 6;
    const float* vbase = qkv + row0 * 3 * D + h * HD + 2 * D + vd;
    float vv[NVI][4];
#pragma unroll
    for (int it = 0; it < NVI; ++it)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int key = (it * NW + vg0) * 4 + q;
        const int kc = key < len ? key : len - 1;
        vv[it][q] = vbase[(long long)kc * 3 * D];
      }
#pragma unroll
    for (int it = 0; it < NVI; ++it) {
      const int vg = it * NW + vg0;
      if (vg < nkb * 8) {
        float vm[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) vm[q] = vg * 4 + q < len ? vv[it][q] : 0.f;
        unsigned h0, l0, h1, l1;
        split16_pair(vm[0], vm[1], h0, l0);
        split16_pair(vm[2], vm[3], h1, l1);
        *reinterpret_cast<U2*>(Vh + vd * VST + vg * 2) = U2{h0, h1};
        *reinterpret_cast<U2*>(Vl + vd * VST + vg * 2) = U2{l0, l1};
      }
    }
  }
  __syncthreads();

  for (int qt = wave; qt < nkt; qt += NW) {
    int qrow = qt * 16 + r;
    qrow = qrow < len ? qrow : len - 1;
    const float* qp = qkv + (row0 + qrow) * 3 * D + h * HD + g * 8;
    U4 qh[2], ql[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const F4 t0 = ld4(qp + c * 32), t1 = ld4(qp + c * 32 + 4);
      constexpr float qs = 0.125f * 1.44269504088896340736f;      // head_dim^-0.5 and log2(e): the softmax runs on 2^x
      const float x[8] = {t0.x * qs, t0.y * qs, t0.z * qs, t0.w * qs, t1.x * qs, t1.y * qs, t1.z * qs, t1.w * qs};
      split_hi_lo_x8(x, qh[c], ql[c]);
    }
    f32x4 s[2 * NKB];
#pragma unroll
    for (int kt = 0; kt < 2 * NKB; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kt < NKT && kt <= qt) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const U4 kh = *reinterpret_cast<const U4*>(Kh + (kt * 16 + r) * KST + c * 16 + g * 4);
          const U4 kl = *reinterpret_cast<const U4*>(Kl + (kt * 16 + r) * KST + c * 16 + g * 4);
          s[kt] = mfma_x3_16x16x32(kl, qh[c], s[kt]);
          s[kt] = mfma_x3_16x16x32(kh, ql[c], s[kt]);
          s[kt] = mfma_x3_16x16x32(kh, qh[c], s[kt]);
        }
      }
    }
    const int query = qt * 16 + r;
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2 * NKB; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt * 16 + g * 4 + i;
        const bool valid = kt <= qt && key < len && (key <= query || query >= len);
        s[kt][i] = valid ? s[kt][i] : -INFINITY;
        m = fmaxf(m, s[kt][i]);
      }
    m = max_groups(m);
    float den = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2 * NKB; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float e = fast_exp2(s[kt][i] - m);
        s[kt][i] = e;
        den += e;
      }
    den = sum_groups(den);
    const float inv = 1.0f / den;
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      if (2 * kb <= qt && kb < nkb) {
        const float pf[8] = {s[2 * kb][0] * inv, s[2 * kb][1] * inv, s[2 * kb][2] * inv, s[2 * kb][3] * inv,
                             s[2 * kb + 1][0] * inv, s[2 * kb + 1][1] * inv, s[2 * kb + 1][2] * inv, s[2 * kb + 1][3] * inv};
        U4 ph, pl;
        split_hi_lo_x8_unit(pf, ph, pl);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const unsigned* vh = Vh + (dt * 16 + r) * VST + kb * 16 + g * 2;
          const unsigned* vl = Vl + (dt * 16 + r) * VST + kb * 16 + g * 2;
          const U2 a0 = *reinterpret_cast<const U2*>(vh), a1 = *reinterpret_cast<const U2*>(vh + 8);
          const U2 b0 = *reinterpret_cast<const U2*>(vl), b1 = *reinterpret_cast<const U2*>(vl + 8);
          const U4 vhh = U4{a0.x, a0.y, a1.x, a1.y}, vll = U4{b0.x, b0.y, b1.x, b1.y};
          oacc[dt] = mfma_x3_16x16x32(pl, vhh, oacc[dt]);
          oacc[dt] = mfma_x3_16x16x32(ph, vll, oacc[dt]);
          oacc[dt] = mfma_x3_16x16x32(ph, vhh, oacc[dt]);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = qt * 16 + g * 4 + i;
        if (q < len) o[(row0 + q) * D + h * HD + dt * 16 + r] = oacc[dt][i];
      }
  }
}

}  // namespace mld
