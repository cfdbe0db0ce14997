// The reverse-diffusion loop of ONE bs-64 request (up to 128 motions per launch) as one persistent launch of CLUSTERS: 24 or 12 workgroups per 8 motions.
//
// Why it exists.  The metric's literal configuration -- one MLD.forward of 64 prompts (mld.py:216-265,290-360) -- ran on
// the launch-per-GEMM family (tile32.hpp): 2 052 dependent launches of ~5.5 us, 12.3 ms per batch.  The sample-major loop (loop_fused.hpp)
// does not help there: 8 workgroups, each streaming all 30 MB of weights per step, take its flat 19 ms.  What was measured first
// (tools/loopbench/sync_bench.hip, profiles/r05_sync_bench.json): a hand-off between workgroups INSIDE a launch -- payload stores, one flag per
// producer, a relaxed poll, L1-bypassing loads -- costs 1.7 us with nothing to move and 2.7 / 3.6 / 3.1 us with 16 / 64 / 48 KB gathered per
// workgroup, against 3.8 / 4.8 / 4.3 us for the same bodies as launches.  So the loop is cut where its all-to-all points are, but the pieces stay
// in one launch:
//
//   cluster = 8 motions = 16 rows of the CFG batch x 3 tokens (the row order of loop_fused.hpp: row = 16 t + c, c < 8 unconditional).
//   member (t, h), t = token 0..2, h = column group 0..CG-1 (CG = 4: every member is a head; CG = 8, calls of up to 64 motions: members h < 4 are the
//   heads and do everything, members h >= 4 skip Ph1 and enter at E1); per layer (cross_attention.py:259-272, forward_post):
//     Ph1  [X of all 48 rows in LDS]  Q of (token t, head h) and K of head h for all three tokens on waves 0-3, V of head h for all three tokens on
//          waves 4-7 (3x redundant over t: the 3-token attention needs them), scores through LDS, softmax + P.V for its 16 rows; then the
//          out-projection SPLIT OVER K BY HEAD: the head's 64 attention dims into all 256 output columns   -> publishes a partial [16][256]
//     E1   the 4 partials of its token, summed in a fixed order + bias + residual -> norm1, one row per wave (in-wave statistics)   64 KB
//     Ph2  linear1 + GELU for hidden columns [1024 h / CG, + 1024 / CG)                      -> publishes its slice of H[16][1024] as a split-f16 image
//     E2   gather the hidden activation of its token from (t, *)                                  64 KB
//     Ph3  linear2 for output columns [256 h / CG, + 256 / CG), K = 1024 on two (CG 4) or four (CG 8) groups of waves that meet through LDS; + bias
//          + the norm2 residual from its own norm1 image                                        -> publishes Y[16][256 / CG]
//     E3   gather Y of ALL 48 rows from all members, norm2 -> next layer's X    48 KB
//   (+ per skip connection, cross_attention.py:56-58: norm2 of its own rows only, Linear(cat[x, skip]) for its 16 rows x 256 / CG columns with
//   K split like linear2's, and one more gather of all 48 rows.)  End of a step (encoder.norm, CFG, DDIM:
//   mld_denoiser.py:206, mld.py:339-346) and the next step's token rows are worked out redundantly by every member: no exchange.
//   31 exchanges per step for the 9-layer model instead of 41 launches.
//
// Weights: as in loop_fused.hpp a weight element is used by exactly one wave, so nothing is staged in LDS: `finalize` writes, per column group
// and WAVE, the fragments that wave consumes in consumption order ([fragment][lane][8 words] split-f16: high halves of k = 8g .. 8g + 7 of
// weight row 16 x + r, then the low halves) and every lane streams its 32 bytes per fragment through a 4-deep register ring (6 or 8 spill).  A head
// member streams 512 KB (CG 8) / 768 KB (CG 4) per layer; the phases that stream run at the L2 -> CU fill rate (58 B/clk), the rest of a layer is
// hand-off latency (DESIGN.md 3a has the kernel's own phase stamps).
//
// Hand-offs: cdna_hip_programming.md Guideline 16 form R1 -- write-through (sc1) payload stores, every storing wave drains its memory counter,
// barrier, one lane stores the member's flag (relaxed, agent scope; value = epoch, never reset inside a call; zeroed by clear_cluster_flags_kernel in
// front of the launch -- NOT by a memset node: DESIGN.md 3a), consumers poll the flags of the producers they need with one relaxed load per lane, then
// read with sc1 loads.  PLAIN payload stores are 0.15-0.6 us per exchange cheaper but only visible to consumers behind the SAME L2: WT = false is
// used only when every member of the cluster reports the same HW_REG_XCC_ID (checked in the kernel's first exchange; block b runs on XCD b % 8 in
// practice, not by contract); a cluster that spans XCDs keeps the write-through stores by itself.
// Buffers are double buffered by the parity of the epoch; E3-type waits cover ALL members even where fewer rows are read, which is what
// keeps a fast member from overwriting a buffer a slow one still reads.  Every spin is bounded: a member that waits longer than
// kClTimeoutTicks sets the call's status words, every member that sees it leaves, the latents are poisoned with NaN (counted by the range
// contract's non-finite counter) and the handle leaves the cluster loop (mldhip_numeric_status).  The last member to finish clears the cluster's flag
// line, so every polled word is zero when a call ends.  The launch needs all its workgroups resident together: the engine sizes it to the chip and never
// issues two of them side by side (engine/params.hpp ClusterLane).
#pragma once
#include "loop_fused.hpp"

namespace mld {

#ifndef CL_RING
#define CL_RING 4
#endif
constexpr int kClMembers = 12, kClMembersMax = 24, kClRing = CL_RING, kClFragFloats = 512;   // members: 3 tokens x 4 column groups (x 8: the wide form)
constexpr int kClXs = 264, kClHs = 1032;                       // LDS row strides (words), = 8 mod 16: conflict-free fragment reads
constexpr unsigned kClPlane = 2u * 48u * 256u;                 // one double-buffered [48][256] fp32 exchange tensor (floats)
constexpr unsigned kClSlab = 2u * 12u * 16u * 256u;            // one double-buffered set of per-member partial slabs [3 tokens][4 members][16][256] (floats)
constexpr unsigned kClH1 = 0, kClY = kClPlane, kClZ = 2 * kClPlane, kClH = 3 * kClPlane, kClPO = kClH + 2u * 48u * 1024u;
constexpr unsigned kClXFloats = kClPO + kClSlab;               // exchange region of one cluster: 270 336 floats = 1 056 KB
constexpr int kClAoS = 72;                                     // LDS row stride (words) of the head's attention output image [16][64 columns]
constexpr int kClFlagLine = 32, kClFlagWords = 4 * kClFlagLine; // flag kinds AO, H, Y, Z: 32 words (one 128-byte line) each; word 28 of the Z line counts finished members
enum : int { kFlagAO = 0, kFlagH = 1, kFlagY = 2, kFlagZ = 3 };
constexpr int kClBigFloats = 16 * kClHs;                       // X of all 48 rows ([48][264] = 12 672 words) and the token's hidden activation ([16][1032]) in turn
static_assert(kClBigFloats >= 48 * kClXs, "X and the hidden activation share one region");
constexpr int kClAsFloats = 16 * kClXs;
constexpr int kClScFloats = 3 * 16 * 4, kClRedFloats = 2 * 16 * 8, kClRed2Floats = 6 * 64 * 4, kClCtlFloats = 16;
constexpr int kClLdsFloats = kClBigFloats + kClAsFloats + kLfLatFloats + 2 * kLfPrmFloats + kClScFloats + kClRedFloats + kClRed2Floats + kClCtlFloats;
constexpr int kClLdsBytes = kClLdsFloats * 4;                  // 125 760 B: one workgroup per CU
constexpr int kClMaxClusters = 16;                             // two clusters per XCD (32 CUs): 128 motions per launch
constexpr int kClMaxCall = 2 * 8 * kClMaxClusters;             // motions per call the engine serves with (two) cluster launches

struct ClFrag { long long src; int ld; int pad; };            // element [row0][k0] of a weight (floats into the arena), row stride

struct ClusterArgs {
  const float* stream;        // per column group and wave: [fragments of a step + kClRing][64 lanes][8 words]
  const unsigned* wave_off;   // [column group][wave] (32 or 64 words in device memory): float offset of that wave's fragment sequence
  const float* small;         // loop_fused.hpp's packed small parameters (kLs*)
  const float* T1;            // [n][256] time-token rows
  const float* TP;            // [2B][256] condition-token rows, unconditional half first
  const float* init_lat;      // [B][256]
  float* lat;                 // [B][256]
  float* park;                // [workgroup][nb][16][256] parked skip rows of the member's own token
  const float* ddim;          // [n][4]
  float* xbuf;                // [clusters][kClXFloats] exchange regions
  unsigned* flags;            // [clusters][kClFlagWords], zeroed in front of the launch
  unsigned* status;           // [0]: 0 ok, 1 a wait timed out; [1]: clusters that span XCDs (plain stores asked for, write-through used); both cleared per launch.  [2]: a wait timed out in SOME launch since the host last looked (sticky)
  int B, L, n, ncl;           // B: motions of the CALL (the condition rows' pitch); this launch serves motions [s_base, s_end)
  int s_base = 0, s_end = 0;
  unsigned* host_status = nullptr;   // pinned host word (or NULL): set with the sticky status word, read by the host at the start of the next call without a device synchronisation
  unsigned timeout = 0;       // wait bound: 100 MHz ticks (GPU) / poll iterations (simulator); kClTimeoutTicks unless a test shortens it
  int mute = -1;              // hooks builds (fault injection, tests): this member never raises its first flag -- everybody who waits for it runs into the bound
  unsigned long long* trace = nullptr;   // CL_TRACE builds (tools/loopbench only): [workgroup][wave][16] shader cycles per phase, summed over steps and layers
  int xslots;                 // blocks per launch row: 8 on the GPU (block b runs on XCD b % 8: a cluster's members share the slot), min(clusters, 8) on the simulator
  float guidance, init_sigma;
  const float* eta = nullptr;        // den_cluster_eta_kernel: [n][2] DdimEta per step
  const NoiseKey* keys = nullptr;    // ... [B] noise key per motion of the call
  const TrajRow* traj = nullptr;     // mldhip_sample_many_traj: [B] trajectory entry per motion of the call, or NULL; member 0 stores, as with `lat`
  const StartRow* starts = nullptr;  // den_cluster_from_kernel / den_cluster_from_eta_kernel: [B] start entry per motion of the call
};

#if defined(MLDHIP_SIM)
constexpr unsigned kClTimeoutTicks = 1u << 26;                 // poll iterations
#else
constexpr unsigned kClTimeoutTicks = 20000000u;                // 100 MHz ticks: 200 ms
#endif

// finalize-time: one fragment = 16 weight rows x 32 k as the split-f16 operand pair of lane (r, g): high halves of W[row0 + r][k0 + 8g .. + 7], then the low halves
__global__ __launch_bounds__(64) void pack_cluster_frags_kernel(const float* __restrict__ arena, const ClFrag* __restrict__ frags, float* __restrict__ out) {
  const ClFrag f = frags[blockIdx.x];
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const float* src = arena + f.src + (long long)r * f.ld + 8 * g;
  const F4 a = ld4(src), b = ld4(src + 4);
  U4 hi, lo;
  split16_pair(a.x, a.y, hi.x, lo.x);
  split16_pair(a.z, a.w, hi.y, lo.y);
  split16_pair(b.x, b.y, hi.z, lo.z);
  split16_pair(b.z, b.w, hi.w, lo.w);
  float* dst = out + (long long)blockIdx.x * kClFragFloats + lane * 8;
  *reinterpret_cast<U4*>(dst) = hi;
  *reinterpret_cast<U4*>(dst + 4) = lo;
}

// every polled word zero at the start of a call (Guideline 16 "Re-initialise every call"): a kernel of the call's own stream, not a memset node
__global__ __launch_bounds__(256) void clear_cluster_flags_kernel(unsigned* __restrict__ flags, int words) {
  for (int i = threadIdx.x; i < words; i += 256) flag_store(flags + i, 0u);
}

// hooks builds (option "cluster_stale"): one polled word holds an epoch no fresh launch can hold -- the entry check's test
__global__ void poke_cluster_flag_kernel(unsigned* __restrict__ word, unsigned v) { flag_store(word, v); }

// grid = 12 xslots x ceil(clusters / xslots), xslots = 8: block b -> XCD slot x = b % 8, index i = b / 8 -> cluster x + 8 (i / 12), member i % 12.  block = 512.
// WT = true: write-through (sc1) payload stores whatever the placement.  WT = false: every cluster whose twelve members report the same XCC id stores its
// payloads plain (served from the shared L2); a cluster that spans XCDs falls back to write-through by itself.
// CG = column groups per token: 4 (12 members: every member is a head) or 8 (24 members, calls of up to 8 clusters: the feed-forward block on twice the CUs --
// members (t, h < 4) are the heads and do everything, members (t, h >= 4) skip Ph1 and enter at E1; linear1 = 128 hidden columns per member, linear2 and the
// skip linear = 32 output columns per member with K on four wave pairs).
template <bool WT, int CG>
__global__ __launch_bounds__(512, 2) void den_cluster_kernel(ClusterArgs p) {
  constexpr bool ETA = false, FROM = false;
#include "loop_cluster_body.hpp"
}

// Stochastic DDIM (eta > 0): the same body with the step's second table row and sigma z added at the DDIM update, one Philox call per lane and step
// (include/mldhip.h "Noise contract").  The body is textually shared, not an inlined function: that keeps the eta = 0 kernel's machine code exactly
// what it was (an always-inlined body schedules it differently).
template <bool WT, int CG>
__global__ __launch_bounds__(512, 2) void den_cluster_eta_kernel(ClusterArgs p) {
  constexpr bool ETA = true, FROM = false;
#include "loop_cluster_body.hpp"
}

// The from-forms (mldhip_sample_many_from): per-motion start states and first steps from p.starts, flag epochs counted from the cluster's own first step
// (loop_cluster_body.hpp FROM).  Kernels of their own next to the two above, which keep their machine code.
template <bool WT, int CG>
__global__ __launch_bounds__(512, 2) void den_cluster_from_kernel(ClusterArgs p) {
  constexpr bool ETA = false, FROM = true;
#include "loop_cluster_body.hpp"
}
template <bool WT, int CG>
__global__ __launch_bounds__(512, 2) void den_cluster_from_eta_kernel(ClusterArgs p) {
  constexpr bool ETA = true, FROM = true;
#include "loop_cluster_body.hpp"
}

}  // namespace mld
