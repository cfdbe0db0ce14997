// Post-norm feed-forward block of a decoder / encoder layer, split-f16 operands:
//   Y = LayerNorm(X + linear2(gelu(linear1(X))))        (cross_attention.py:340-343 decoder layer, :268-271 encoder layer)
// for D = 256, FF = 1024, structured by what the sample-major loop taught
// (loop_fused.hpp): a weight element is used by exactly one wave (wave w owns columns 16w .. 16w + 15 of every 128-column block,
// ALL row tiles of the strip), so weights never go through LDS: every lane loads its two 16-byte MFMA operands per item
// straight from a fragment-ordered stream (`finalize` re-packs linear1 / linear2 per layer in consumption order) into a register
// ring -- no weight staging, no barrier per item (round 2's LDS-staged form, retired in round 4: 128 barriers and 2 MB of LDS stores +
// 4 MB of LDS reads per workgroup; 1.72 vs 1.10 ms per launch at 2 048 motions).  What is left in LDS is the strip itself -- RT x 16 rows of X as a split image -- and one 128-wide block of the
// hidden activation at a time.  RT = 6 (96 rows): 2 MB of weights per 96 rows instead of per 64, i.e. 1.5x less L2 -> CU traffic;
// RT = 3 (48 rows, 80 KB of LDS, 128 registers): two workgroups per CU, four waves per SIMD -- one workgroup's barriers and GELU
// stretches run under the other's matrix instructions; measured 2 % faster over the decoder than RT = 6.
//
// Pipeline over the eight hidden blocks:   run1(0); gelu(0)
//   hb = 1..7:  W(hb-1) | run1(hb) | { run2(hb-1) || gelu(hb) }        W = barrier, write H block to LDS, barrier
//   W(7) | run2(7) | bias + residual + LayerNorm -> Y
// run1 = linear1 of a block (8 items), run2 = linear2's share of a block (8 items: 4 K chunks x 2 column blocks, A fragments
// shared), gelu = bias + erf-GELU + hi/lo split of the block's accumulators into registers: pure VALU, issued between the
// matrix instructions of run2, which do not depend on it.  The H block is single-buffered: it is rewritten only between the
// two barriers of W, after every wave has left run2 of the previous block.
//
// Summation order differs from the two staged GEMMs of gemm.hpp (the "ffn_strip" = 0 path), so results agree to fp32 rounding, not bitwise.
#pragma once
#include "loop_fused.hpp"

namespace mld {

struct FfnArgs {
  const float* X = nullptr;        // [M][256] fp32: block input and residual
  const float* W1 = nullptr;       // split image of linear1.weight [1024][256]
  const float* b1 = nullptr;       // [1024]
  const float* W2 = nullptr;       // split image of linear2.weight [256][1024]
  const float* b2 = nullptr;       // [256]
  const float* gamma = nullptr;    // LayerNorm after the residual
  const float* beta = nullptr;
  float* Y = nullptr;              // [M][256]
  int M = 0;
  const int* skip_lens = nullptr;  // skip row tiles made only of rows (row % rpg) >= skip_lens[row / rpg] (padded frames)
  int skip_rpg = 1;
  // ffn_strip_x3_kernel<RT, true> ("decoder tail": the self-attention out-projection + residual + norm1 + cross-attention vector + norm2 in
  // front of the feed-forward block, one launch; X is not read, the block input is produced in LDS)
  const float* AO = nullptr;       // [M][256] attention output (A operand of the out-projection)
  const float* Wo = nullptr;       // fragment-ordered stream of out_proj.weight (16 items: 8 chunks x [block 0, block 1])
  const float* bo = nullptr;       // [256]
  const float* res = nullptr;      // [M][256] the layer input (residual of norm1)
  const float* g1 = nullptr; const float* be1 = nullptr;      // norm1
  const float* cvec = nullptr; int rpg = 1;                   // + cvec[row / rpg][256] before norm2
  const float* g2 = nullptr; const float* be2 = nullptr;      // norm2
};


constexpr int kFsXs = 264, kFsHs = 136;      // row strides (words), = 8 mod 16 (conflict-free fragment reads)
template <int RT>
constexpr int ffn_strip_lds_bytes() { return (RT * 16 * kFsXs + RT * 16 * kFsHs + 2 * 8 * RT * 16 + RT * 16) * 4; }   // RT = 6: 160 128 B; RT = 4: 106 752 B; RT = 3: 80 064 B (two per CU)

// items of one layer's stream: run1(0), then [run1(hb), run2(hb - 1)] for hb = 1..7, then run2(7); 128 items of 16 KB
constexpr int kFfnStripItems = 128;

// grid = ceil(M / (16 RT)); block = 512.  p.W1 = the layer's fragment-ordered stream (W2 unused).
// TAIL: the rest of a decoder layer behind its self-attention in ONE launch -- out-projection (16 more items, from the row-strip GEMM's
// stream of out_proj.weight) + residual + norm1 + cross-attention vector + norm2 produce the block input in LDS instead of reading it:
// the layer's H1 tensor (M x 256 fp32, written by one launch and read by the next) disappears, 0.8 GB of the decoder's 5.3 GB of HBM
// traffic per layer at 2 048 motions -- and the decoder's row-strip kernels are bound by exactly that traffic (~3.1 TB/s, r03).
// SWZ: the strip's and the hidden block's images are stored XOR-swizzled by the row, exactly as in the persistent loop (loop_fused.hpp
// SWZ: physical word = logical word ^ 4 ((row >> 2) & 3); 8-byte row stores 4-way -> 2-way, fragment reads stay conflict free).
// row of the attention output that holds row m = (sample s, frame t) of decoder layer 0: the same frame of the sample's length representative
__device__ __forceinline__ size_t l0_source_row(int m, int rpg, const int* __restrict__ rep) {
  const int s = m / rpg;
  return (size_t)rep[s] * rpg + (m - s * rpg);
}

// L0 (dec_tail_l0_x3_kernel, decoder layer 0 under "dec_lean"): the layer input is the positional table, the same for every sample, so
//   - the residual of norm1 is p.res[row % rpg] (p.res = the [rpg][256] table itself: no [M][256] copy of it exists), and
//   - the attention output of row (s, t) is read from the rows of rep[s], the first sample of the same length (length_reps_kernel): layer 0's
//     attention output depends on (t, length) only, and only representatives compute it.
// Both are compile-time forms of that one entry; the body is ONE text, ffn_strip_body.hpp, included by both kernels (as loop_cluster.hpp does): the
// kernels of layers 1 .. 8 keep their addressing and their machine code to the instruction (tools/kernel_hashes.py).
template <int RT, bool TAIL = false, bool SWZ = false>
__global__ __launch_bounds__(512, RT <= 3 ? 4 : 2) void ffn_strip_x3_kernel(FfnArgs p) {
  constexpr bool L0 = false;
  constexpr const int* rep = nullptr;
#include "ffn_strip_body.hpp"
}

// decoder layer 0's tail under "dec_lean" (see L0 above): the body of ffn_strip_x3_kernel<3, true, true>, p.res = the positional table [p.rpg][256]
__global__ __launch_bounds__(512, 4) void dec_tail_l0_x3_kernel(FfnArgs p, const int* __restrict__ rep) {
  constexpr int RT = 3;
  constexpr bool TAIL = true, SWZ = true, L0 = true;
#include "ffn_strip_body.hpp"
}

}  // namespace mld
