// The SMPL body model (engine/path_smpl.hpp; mldhip_smpl_forward): rot6d features [frames][150] -> 24 joints and V vertices per frame.
//
// Replaces: Rotation2xyz (mld/transforms/rotation2xyz.py:10-114) over smplx's SMPLLayer with betas = 0, as the two lambdas of MLD.__init__ call it
// (mld/models/modeltype/mld.py:118-143): rotation_6d_to_matrix, the 24-joint kinematic chain, the 207 pose-corrective blend shapes and linear-blend
// skinning.  include/mldhip.h has the math and the padded-frame rule.
//
// Two kernels.  Frames are numbered b T + t over the call and cut into TILES of 16 (the row count of v_mfma_f32_16x16x4_f32).
//   smpl_chain_kernel   one lane per frame: R_j of the 24 slots, the chain G_i = G_parent(i) [R_i | J_i - J_parent(i)] (parents' matrices are looked up in
//                       LDS columns the lane owns: no barrier), the joints output, and the vertex kernel's operands in the layouts its matrix instructions
//                       read without any index math: pf [tile][k 0..207][frame 16] (k = 207 is the zero that pads K to 52 steps of 4) and
//                       A [tile][entry 12][joint 24][frame 16] (entry = row 4 + column of [G.R | G.t - G.R J]), plus aux [frame][4] = {state, translation}.
//   smpl_verts_kernel   the hot path.  A workgroup stages the pf / A tiles of 16 FT frames in LDS once and its four waves walk 16-vertex blocks.  Per block
//                       and frame tile a wave holds 3 accumulators (x, y, z offsets: pf . posedirs, 52 exact-fp32 MFMAs each) and 12 more for the blended
//                       skinning matrix sum_j W[v][j] A_j (a [16 frames x 24 joints] x [24 x 16 vertices] product per entry: 6 MFMAs each, dense weights
//                       cost what sparse ones do).  All 15 tiles share one layout -- frame (lane >> 4) 4 + register, vertex lane & 15 -- so the
//                       skinning of a (frame, vertex) is 12 FMAs on the lane's own registers, followed by the store and the non-finite count.  The
//                       [frames][3V] offsets exist in registers only.
// posedirs, the weights and the template are re-laid per 16-vertex block at finalize (smpl_relay_*_kernel below): the B operand of step s and
// coordinate c is the 64 consecutive floats at ((blk 52 + s) 3 + c) 64, vertices behind V zero.
// Exact fp32 in every precision mode: posedirs sits at 1e-3 .. 1e-2, where the low half of a split-f16 image is a half subnormal.
#pragma once
#include "rt.hpp"

namespace mld {

constexpr int kSmplJoints = 24, kSmplFeats = 150, kSmplSlots = 25, kSmplK = 207, kSmplKP = 208, kSmplSteps = kSmplKP / 4;
constexpr int kSmplPfTile = kSmplKP * 16, kSmplATile = 12 * kSmplJoints * 16;      // floats per 16-frame tile
enum : int { SMPL_TRANS_JOINTS = 1, SMPL_TRANS_VERTS = 2 };
// aux[frame][0]: 0 = behind the call's last frame (nothing is stored), 1 = valid, 2 = padded (t >= len: zeros, plus the translation term when asked)

__device__ __forceinline__ float nonfinite_f(float x) { return ((__builtin_bit_cast(unsigned, x) & 0x7F800000u) == 0x7F800000u) ? 1.f : 0.f; }
__device__ __forceinline__ void add_count(unsigned* counter, float bad) {
  bad = sum64(bad);
  if ((threadIdx.x & 63) == 0 && bad > 0.f) {
#if defined(MLDHIP_SIM)
    *counter += (unsigned)bad;
#else
    atomicAdd(counter, (unsigned)bad);
#endif
  }
}

struct SmplChainArgs {
  const float* feats;       // [B][T][150]
  const int* lens;          // [B]
  const float* J;           // [24][3] rest joints
  const float* Jrel;        // [24][3] J_i - J_parent(i) (row 0: J_0)
  const int* parents;       // [24]
  float* joints;            // [B][T][24][3] or NULL
  float* pf;                // [tiles][208][16]
  float* A;                 // [tiles][12][24][16]
  float* aux;               // [tiles x 16][4]
  unsigned* counter;
  int T, frames;            // frames per motion; B x T
  int f0, n;                // this launch covers frames f0 .. f0 + n - 1 of the call (f0 a multiple of 16); workspace tile 0 = frame f0
  int flags;
};

// grid ceil(n / 64) (n rounded up to whole tiles), block 64
__global__ __launch_bounds__(64) void smpl_chain_kernel(SmplChainArgs p) {
  __shared__ float G[kSmplJoints * 12 * 64];      // [joint][entry][lane]: every lane reads and writes its own column only
  const int lane = threadIdx.x;
  const int lf = blockIdx.x * 64 + lane;                       // frame inside the launch
  const int tiles_n = (p.n + 15) / 16 * 16;
  float bad = 0.f;
  if (lf < tiles_n) {
    const int fr = p.f0 + lf, tile = lf >> 4, fi = lf & 15;
    float* pf = p.pf + (long long)tile * kSmplPfTile + fi;
    float* A = p.A + (long long)tile * kSmplATile + fi;
    float* aux = p.aux + (long long)lf * 4;
    const bool inside = lf < p.n && fr < p.frames;
    const int b = inside ? fr / p.T : 0, t = inside ? fr - b * p.T : 0;
    const bool valid = inside && t < p.lens[b];
    if (!valid) {
      // a padded frame or a row behind the call: zero operands (their products are never stored); padded frames keep their translation term
      for (int k = 0; k < kSmplKP; ++k) pf[k * 16] = 0.f;
      for (int q = 0; q < 12 * kSmplJoints; ++q) A[q * 16] = 0.f;
      float d[3] = {0.f, 0.f, 0.f};
      if (inside) {
        const float* f = p.feats + (long long)fr * kSmplFeats;
        const float* f0 = p.feats + (long long)b * p.T * kSmplFeats;
        for (int c = 0; c < 3; ++c) d[c] = f[c * kSmplSlots + 24] - f0[c * kSmplSlots + 24];
        if (p.joints) {
          float* jo = p.joints + (long long)fr * kSmplJoints * 3;
          for (int q = 0; q < kSmplJoints * 3; ++q) {
            const float v = (p.flags & SMPL_TRANS_JOINTS) ? 0.f + d[q % 3] : 0.f;
            bad += nonfinite_f(v);
            jo[q] = v;
          }
        }
      }
      aux[0] = inside ? 2.f : 0.f; aux[1] = d[0]; aux[2] = d[1]; aux[3] = d[2];
    } else {
      const float* f = p.feats + (long long)fr * kSmplFeats;
      const float* f0 = p.feats + (long long)b * p.T * kSmplFeats;
      float d[3];
      for (int c = 0; c < 3; ++c) d[c] = f[c * kSmplSlots + 24] - f0[c * kSmplSlots + 24];
      aux[0] = 1.f; aux[1] = d[0]; aux[2] = d[1]; aux[3] = d[2];
      float* jo = p.joints ? p.joints + (long long)fr * kSmplJoints * 3 : nullptr;
      float root[3] = {0.f, 0.f, 0.f};
      for (int j = 0; j < kSmplJoints; ++j) {
        // rotation_6d_to_matrix: rows b1, b2, b3
        const float a1[3] = {f[j], f[kSmplSlots + j], f[2 * kSmplSlots + j]};
        const float a2[3] = {f[3 * kSmplSlots + j], f[4 * kSmplSlots + j], f[5 * kSmplSlots + j]};
        const float n1 = fmaxf(sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12f);
        const float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
        const float dt = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
        const float u[3] = {a2[0] - dt * b1[0], a2[1] - dt * b1[1], a2[2] - dt * b1[2]};
        const float n2 = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
        const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
        const float R[9] = {b1[0], b1[1], b1[2], b2[0], b2[1], b2[2],
                            b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
        if (j >= 1) {
#pragma unroll
          for (int q = 0; q < 9; ++q) pf[((j - 1) * 9 + q) * 16] = R[q] - ((q == 0 || q == 4 || q == 8) ? 1.f : 0.f);
        }
        const float* jr = p.Jrel + j * 3;
        float g[12];                                            // [G.R | G.t], row-major 3 x 4
        if (j == 0) {
#pragma unroll
          for (int r = 0; r < 3; ++r) { g[r * 4] = R[r * 3]; g[r * 4 + 1] = R[r * 3 + 1]; g[r * 4 + 2] = R[r * 3 + 2]; g[r * 4 + 3] = jr[r]; }
        } else {
          const float* gp = G + p.parents[j] * 12 * 64 + lane;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const float p0 = gp[(r * 4) * 64], p1 = gp[(r * 4 + 1) * 64], p2 = gp[(r * 4 + 2) * 64], p3 = gp[(r * 4 + 3) * 64];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[r * 4 + c] = p0 * R[c] + p1 * R[3 + c] + p2 * R[6 + c];
            g[r * 4 + 3] = p0 * jr[0] + p1 * jr[1] + p2 * jr[2] + p3;
          }
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) G[(j * 12 + q) * 64 + lane] = g[q];
        if (j == 0) { root[0] = g[3]; root[1] = g[7]; root[2] = g[11]; }
        if (jo) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float v = g[c * 4 + 3] - root[c];
            if (p.flags & SMPL_TRANS_JOINTS) v += d[c];
            bad += nonfinite_f(v);
            jo[j * 3 + c] = v;
          }
        }
        // A_j = [G.R | G.t - G.R J_j]
        const float* Jj = p.J + j * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          A[((r * 4 + 0) * kSmplJoints + j) * 16] = g[r * 4];
          A[((r * 4 + 1) * kSmplJoints + j) * 16] = g[r * 4 + 1];
          A[((r * 4 + 2) * kSmplJoints + j) * 16] = g[r * 4 + 2];
          A[((r * 4 + 3) * kSmplJoints + j) * 16] = g[r * 4 + 3] - (g[r * 4] * Jj[0] + g[r * 4 + 1] * Jj[1] + g[r * 4 + 2] * Jj[2]);
        }
      }
      pf[kSmplK * 16] = 0.f;
    }
  }
  if (p.joints) add_count(p.counter, bad);
}

struct SmplVertArgs {
  const float* pf;          // [tiles][208][16]
  const float* A;           // [tiles][12][24][16]
  const float* aux;         // [tiles x 16][4]
  const float* P;           // [nblk][52][3][64] re-laid posedirs
  const float* W;           // [nblk][24][16] re-laid skinning weights
  const float* vt;          // [nblk][3][16] re-laid template
  float* verts;             // [B][T][V][3]
  unsigned* counter;
  int V, nblk;
  int f0, tiles;            // first frame of the launch, its 16-frame tiles
  int flags;
};

// grid (vertex-block lanes, ceil(tiles / FT)), block 256: wave w of workgroup (x, y) walks blocks 4 x + w, 4 (x + gridDim.x) + w, ... over the FT tiles of y
template <int FT>
__global__ __launch_bounds__(256, 2) void smpl_verts_kernel(SmplVertArgs p) {
  __shared__ __attribute__((aligned(16))) float pf_s[FT * kSmplPfTile];
  __shared__ __attribute__((aligned(16))) float A_s[FT * kSmplATile];
  __shared__ float aux_s[FT * 16 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int tile0 = blockIdx.y * FT;
  const int nt = p.tiles - tile0 < FT ? p.tiles - tile0 : FT;      // tiles this workgroup really has (the others: zero operands, nothing stored)
  {
    const float* src = p.pf + (long long)tile0 * kSmplPfTile;
    for (int i = tid * 4; i < FT * kSmplPfTile; i += 1024) st4(pf_s + i, i < nt * kSmplPfTile ? ld4(src + i) : F4{0.f, 0.f, 0.f, 0.f});
    src = p.A + (long long)tile0 * kSmplATile;
    for (int i = tid * 4; i < FT * kSmplATile; i += 1024) st4(A_s + i, i < nt * kSmplATile ? ld4(src + i) : F4{0.f, 0.f, 0.f, 0.f});
    src = p.aux + (long long)tile0 * 64;
    for (int i = tid; i < FT * 64; i += 256) aux_s[i] = i < nt * 64 ? src[i] : 0.f;
  }
  __syncthreads();
  const int vl = lane & 15, g = lane >> 4;
  float bad = 0.f;
  for (int blk = blockIdx.x * 4 + wave; blk < p.nblk; blk += gridDim.x * 4) {
    f32x4 acc[FT][3], m[FT][12];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[ft][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 12; ++q) m[ft][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // blended skinning matrices: m[entry][frame][vertex] = sum_j A[entry][j][frame] W[j][vertex]
    const float* Wb = p.W + (long long)blk * (kSmplJoints * 16) + lane;
#pragma unroll
    for (int s = 0; s < kSmplJoints / 4; ++s) {
      const float w = Wb[s * 64];
#pragma unroll
      for (int ft = 0; ft < FT; ++ft)
#pragma unroll
        for (int q = 0; q < 12; ++q) m[ft][q] = mfma_f32_16x16x4(A_s[ft * kSmplATile + (q * kSmplJoints + s * 4) * 16 + lane], w, m[ft][q]);
      sched_fence();      // (without it hipcc hoists all 144 LDS reads above the products and spills)
    }
    // pose-corrective offsets: acc[c][frame][vertex] = sum_k pf[frame][k] posedirs[k][3 v + c], one k-ordered chain of 208
    const float* Pb = p.P + (long long)blk * (kSmplSteps * 3 * 64) + lane;
#pragma unroll 4
    for (int s = 0; s < kSmplSteps; ++s) {
      const float b0 = Pb[(s * 3) * 64], b1 = Pb[(s * 3 + 1) * 64], b2 = Pb[(s * 3 + 2) * 64];
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) {
        const float a = pf_s[ft * kSmplPfTile + s * 64 + lane];
        acc[ft][0] = mfma_f32_16x16x4(a, b0, acc[ft][0]);
        acc[ft][1] = mfma_f32_16x16x4(a, b1, acc[ft][1]);
        acc[ft][2] = mfma_f32_16x16x4(a, b2, acc[ft][2]);
      }
    }
    const int v = blk * 16 + vl;
    const float* vtb = p.vt + (long long)blk * 48 + vl;
    const float t0 = vtb[0], t1 = vtb[16], t2 = vtb[32];
    if (v < p.V) {
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int fl = ft * 16 + g * 4 + r;
          const float* ax = aux_s + fl * 4;
          const float state = ax[0];
          if (state == 0.f) continue;
          const float x = t0 + acc[ft][0][r], y = t1 + acc[ft][1][r], z = t2 + acc[ft][2][r];
          float o[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float val = fmaf(m[ft][c * 4][r], x, fmaf(m[ft][c * 4 + 1][r], y, fmaf(m[ft][c * 4 + 2][r], z, m[ft][c * 4 + 3][r])));
            if (state != 1.f) val = 0.f;
            if (p.flags & SMPL_TRANS_VERTS) val += ax[1 + c];
            bad += nonfinite_f(val);
            o[c] = val;
          }
          float* out = p.verts + ((long long)(p.f0 + tile0 * 16 + fl) * p.V + v) * 3;
          out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
        }
      }
    }
  }
  add_count(p.counter, bad);
}

// finalize: posedirs [207][3V] -> P [nblk][52][3][4][16]: element (blk, s, c, kk, vv) = posedirs[4 s + kk][3 (16 blk + vv) + c], zero for k = 207 and v >= V
__global__ __launch_bounds__(256) void smpl_relay_posedirs_kernel(const float* __restrict__ pd, float* __restrict__ out, int V, int nblk) {
  const long long n = (long long)nblk * kSmplSteps * 3 * 64;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int vv = (int)(i & 15), kk = (int)((i >> 4) & 3);
    const long long q = i >> 6;
    const int c = (int)(q % 3), s = (int)((q / 3) % kSmplSteps);
    const long long blk = q / (3 * kSmplSteps);
    const int k = s * 4 + kk;
    const long long v = blk * 16 + vv;
    out[i] = (k < kSmplK && v < V) ? pd[(long long)k * 3 * V + 3 * v + c] : 0.f;
  }
}

// finalize: lbs_weights [V][24] -> W [nblk][24][16] and v_template [V][3] -> vt [nblk][3][16], zero for v >= V
__global__ __launch_bounds__(256) void smpl_relay_small_kernel(const float* __restrict__ lw, const float* __restrict__ vtemp, float* __restrict__ W,
                                                               float* __restrict__ vt, int V, int nblk) {
  const long long nw = (long long)nblk * kSmplJoints * 16, n = nw + (long long)nblk * 48;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (i < nw) {
      const int vv = (int)(i & 15), j = (int)((i >> 4) % kSmplJoints);
      const long long v = i / (kSmplJoints * 16) * 16 + vv;
      W[i] = v < V ? lw[v * kSmplJoints + j] : 0.f;
    } else {
      const long long q = i - nw;
      const int vv = (int)(q & 15), c = (int)((q >> 4) % 3);
      const long long v = q / 48 * 16 + vv;
      vt[q] = v < V ? vtemp[v * 3 + c] : 0.f;
    }
  }
}

}  // namespace mld
