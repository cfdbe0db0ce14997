// Body of den_cluster_kernel / den_cluster_eta_kernel (loop_cluster.hpp), included inside both: in scope are the kernel argument `p` (ClusterArgs) and
// the compile-time constants WT, CG, ETA and FROM.  No include guard on purpose.
// FROM (den_cluster_from_kernel / den_cluster_from_eta_kernel, mldhip_sample_many_from): every motion's start state comes from its StartRow, the cluster's step loop
// begins at step0 = the smallest first step of its real motions (all members read the same eight entries, so they agree), and the flag epochs count from step0 --
// a from-launch holds the epochs a plain launch of n - step0 steps holds, so the entry check, the `mute` injection and the parity of the exchange buffers are unchanged.
  constexpr int kM = 3 * CG;
#if defined(MLDHIP_SIM)
  float* smem = reinterpret_cast<float*>(hipsim::blk().dyn_smem.data());
#else
  extern __shared__ __attribute__((aligned(16))) float smem[];
#endif
  float* Xs = smem;                              // [48][264] layer input, split image; later [16][1032]: the token's hidden activation
  float* As = Xs + kClBigFloats;                 // [16][264] attention output, then norm1 output (own token), split image
  float* lats = As + kClAsFloats;                // [8][256]
  float* prm = lats + kLfLatFloats;              // [2][kLfPrmFloats]
  float* sc = prm + 2 * kLfPrmFloats;            // [3 keys][16 rows][4 waves] partial attention scores
  float* red = sc + kClScFloats;                 // [2 passes][16 rows][8 waves]
  float* red2 = red + kClRedFloats;              // [4 waves][64 lanes][4] K-half partial tiles
  unsigned* ctl = reinterpret_cast<unsigned*>(red2 + kClRed2Floats);
  const int wave = wave_uniform((int)threadIdx.x >> 6);
  unsigned goff = 0;                                       // this lane's running word offset into its wave's fragment stream
  [[maybe_unused]] const int hc_ = (((int)blockIdx.x / p.xslots) % kM) % CG;
  int lane = (int)threadIdx.x & 63, tid = (int)threadIdx.x, r = lane & 15, g = lane >> 4;
  int swz4 = ((r >> 2) & 3) << 2;                          // row swizzle of the operand images (loop_fused.hpp SWZ): XOR of the word offset's bits 2-3
  int gs4 = (g << 2) ^ swz4;                               // this lane's 16-byte group of a half chunk
  // Lane-dependent indices are laundered at the top of every phase: address arithmetic built on them is then redone where it is used instead of
  // being hoisted out of the step / layer loops and held -- i.e. spilled -- across all phases (loop_fused.hpp `opaque`; the first build of this kernel:
  // 256 registers + 544 B of scratch per lane, most of it loop-invariant addresses stored in the prologue)
  auto fresh = [&]() __attribute__((always_inline)) {
#if !defined(MLDHIP_SIM)
    asm volatile("" : "+v"(lane));
#endif
#if defined(CL_EXP) && (CL_EXP & 1)
    goff = p.wave_off[hc_ * 8 + wave] + (unsigned)lane * 8u;      // measurement build (WRONG results, tools/loopbench only): every phase re-reads the step's first fragments -- an L2-resident weight stream
#endif
    tid = wave * 64 + lane;
    r = lane & 15;
    g = lane >> 4;
    swz4 = ((r >> 2) & 3) << 2;
    gs4 = (g << 2) ^ swz4;
  };
  const int bx = (int)blockIdx.x % p.xslots, bi = (int)blockIdx.x / p.xslots;
  const int cluster = bx + p.xslots * (bi / kM), member = bi % kM;
  if (cluster >= p.ncl) return;
  const int tk = member / CG, hc = member % CG;  // token, column group (a head when < 4)
  const bool att = hc < 4;
  constexpr unsigned all_mask = (1u << kM) - 1u;
  const int s0 = p.s_base + cluster * 8, nb = (p.L - 1) / 2;
  const float* sm_fin = p.small + (long long)p.L * kLsLayer + nb * 256;
  const XBuf xb = xbuf_make(p.xbuf + (size_t)cluster * kClXFloats, kClXFloats * 4u);
  unsigned* flags = p.flags + (size_t)cluster * kClFlagWords;

#ifdef CL_TRACE
  unsigned long long ph[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tph = clock_light();
#define CL_STAMP(k) do { const unsigned long long t_ = clock_light(); ph[k] += t_ - tph; tph = t_; } while (0)
#else
#define CL_STAMP(k) do { } while (0)
#endif
  // ---- waiting for members: wave 0, lane m polls member m's flag of `kind`; bounded; the verdict reaches everybody through LDS + barrier
  auto wait_flags = [&](int kind, unsigned mask, unsigned epoch) -> bool {
    if (wave == 0) {
      const unsigned* f = flags + kind * kClFlagLine + (lane < kM ? lane : 0);
      const bool need = lane < kM && ((mask >> lane) & 1u);
      bool ok = true;
#if defined(MLDHIP_SIM)
      unsigned long long it = 0;
#else
      const unsigned long long ts = realtime_100mhz();
      unsigned it = 0;
#endif
      for (;;) {
        const bool ready = !need || flag_load(f) >= epoch;
        if (!wave_any(!ready)) break;
        spin_pause();
#if defined(MLDHIP_SIM)
        if (wave_any(++it > p.timeout || flag_load(p.status) != 0u)) { ok = false; break; }      // (wave-uniform exit: the lanes meet again in wave_any)
#else
        if ((++it & 63u) == 0u) {
          const bool late = realtime_100mhz() - ts > p.timeout;
          if (wave_any(late || flag_load(p.status) != 0u)) { ok = false; break; }
        }
#endif
      }
      poll_fence();
      if (lane == 0) {
        if (!ok) { flag_store(p.status, 1u); flag_store(p.status + 2, 1u); host_flag_store(p.host_status, 1u); }      // [2] is sticky: cleared by the host once it has acted on it
        ctl[0] = ok ? 1u : 0u;
      }
    }
    __syncthreads();
    return ctl[0] != 0u;
  };
  // ---- one wave waits for ONE member (the producer of the slice this wave gathers): no workgroup barrier between the poll and the loads; a timeout is left in ctl[2] for
  // everybody to see behind the next barrier (12-workgroup form's E2: -1.6 % per layer; on the 24-workgroup form eight waves polling eight words of one line lose 1.5 %)
  auto wait_one = [&](int kind, int m, unsigned epoch) {
    const unsigned* f = flags + kind * kClFlagLine + m;
    bool ok = true;
#if defined(MLDHIP_SIM)
    unsigned long long it = 0;
#else
    const unsigned long long ts = realtime_100mhz();
    unsigned it = 0;
#endif
    for (;;) {
      if (!wave_any(flag_load(f) < epoch)) break;
      spin_pause();
#if defined(MLDHIP_SIM)
      if (wave_any(++it > p.timeout || flag_load(p.status) != 0u)) { ok = false; break; }
#else
      if ((++it & 63u) == 0u) {
        const bool late = realtime_100mhz() - ts > p.timeout;
        if (wave_any(late || flag_load(p.status) != 0u)) { ok = false; break; }
      }
#endif
    }
    poll_fence();
    if (!ok && lane == 0) { flag_store(p.status, 1u); flag_store(p.status + 2, 1u); host_flag_store(p.host_status, 1u); ctl[2] = 1u; }
  };
  auto publish = [&](int kind, unsigned epoch) __attribute__((always_inline)) {
#if defined(CL_EXP) && (CL_EXP & 2)
    // measurement build (WRONG results, tools/loopbench only): the flag goes up without waiting for the payload stores or for the other waves -- the upper bound of what
    // cheaper publishes (per-wave flags, no workgroup barrier) could buy (profiles/r06_loop_experiments.json)
    if (tid == 0) flag_store(flags + kind * kClFlagLine + member, epoch);
    return;
#endif
    drain_stores();
    __syncthreads();
    if (tid == 0 && !(member == p.mute && epoch == 1u)) flag_store(flags + kind * kClFlagLine + member, epoch);
  };
  auto give_up = [&]() {           // a wait failed: poison this cluster's latents (member 0), leave
    if (member == 0) {
      const int c = tid >> 6, c4 = tid & 63;
      const float qnan = __builtin_nanf("");
      if (s0 + c < p.s_end) {
        st4(p.lat + (long long)(s0 + c) * 256 + c4 * 4, F4{qnan, qnan, qnan, qnan});
        if (p.traj) {                  // ... and the last trajectory row of its motions: traj[n - 1] == lat also behind a failed launch
          const TrajRow tr = p.traj[s0 + c];
          if (tr.row0) st4_global(tr.row0 + (long long)(p.n - 1) * tr.step_stride + c4 * 4, F4{qnan, qnan, qnan, qnan});
        }
      }
    }
  };

  // Entry check (advisor r5): what a FRESH launch can find in this cluster's polled words is bounded -- a member is at most one exchange ahead of member 0 (it needs
  // member 0's share to go on), so the AO / H / Y lines hold epochs <= 2, the Z line the XCC census (<= 16) and its finish counter 0.  Anything else is what a previous
  // launch left behind and the clear in front of this one did not remove (r05: a captured memset node): the launch is failed (status words, NaN latents, counted, fallback;
  // the other members see the status word in their waits) instead of consuming the words as "ready".
  if (member == 0) {
    if (wave == 0) {
      const unsigned a = flag_load(flags + lane), b = flag_load(flags + 64 + lane);
      const unsigned lim = lane < 32 ? 2u : (lane == 32 + 28 ? 0u : 17u);
      const bool stale = wave_any(a > 2u || b > lim);
      if (lane == 0) {
        ctl[0] = stale ? 0u : 1u;
        if (stale) { flag_store(p.status, 1u); flag_store(p.status + 2, 1u); host_flag_store(p.host_status, 1u); }
      }
    }
    __syncthreads();
    if (ctl[0] == 0u) { give_up(); return; }
  }

  // ---- weight ring: this lane's two MFMA operands (32 bytes) of the wave's next kClRing fragments
  const unsigned wbase = p.wave_off[hc * 8 + wave] + (unsigned)lane * 8u;
  goff = wbase;
  F4 ring[kClRing][2];
  auto gload = [&](int slot) __attribute__((always_inline)) {
    const float* s = p.stream + goff;
    ring[slot][0] = ld4(s);
    ring[slot][1] = ld4(s + 4);
    goff += (unsigned)kClFragFloats;
#if !defined(MLDHIP_SIM)
    asm volatile("" : "+v"(goff));
#endif
  };
  // three tokens against one fragment (loop_fused.hpp mma_item); one token against one fragment on two accumulators (cross terms / high x high)
  // (`more` = false for the last kClRing fragments in front of a publish: the ring is refilled BEHIND the flag store, under the wait -- a drain of the
  // payload stores would otherwise wait for the look-ahead loads issued just before them: the memory counter is in order)
  auto mma3 = [&](int j, const F4 (&x)[3][2], f32x4 (&acc)[3], bool more = true) __attribute__((always_inline)) {
    const int slot = j % kClRing;
    const U4 wh = __builtin_bit_cast(U4, ring[slot][0]), wl = __builtin_bit_cast(U4, ring[slot][1]);
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = mfma_x3_16x16x32(wh, __builtin_bit_cast(U4, x[t][1]), acc[t]);
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = mfma_x3_16x16x32(wl, __builtin_bit_cast(U4, x[t][0]), acc[t]);
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = mfma_x3_16x16x32(wh, __builtin_bit_cast(U4, x[t][0]), acc[t]);
    if (more) gload(slot);
    sched_fence();
  };
  auto mma1 = [&](int j, const F4 (&x)[2], f32x4& a0, f32x4& a1, bool more = true) __attribute__((always_inline)) {
    const int slot = j % kClRing;
    const U4 wh = __builtin_bit_cast(U4, ring[slot][0]), wl = __builtin_bit_cast(U4, ring[slot][1]);
    a0 = mfma_x3_16x16x32(wh, __builtin_bit_cast(U4, x[1]), a0);
    a1 = mfma_x3_16x16x32(wh, __builtin_bit_cast(U4, x[0]), a1);
    a0 = mfma_x3_16x16x32(wl, __builtin_bit_cast(U4, x[0]), a0);
    if (more) gload(slot);
    sched_fence();
  };
  auto refill = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kClRing; ++j) gload(j);
  };
  auto frag = [&](const float* buf, int st, int row, int kc, F4 (&x)[2]) __attribute__((always_inline)) {
    const float* a = buf + row * st + 32 * kc + gs4;
    x[0] = ld4(a);
    x[1] = ld4(a + 16);
  };
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  bool wt_ = true;                                         // payload stores write-through (set after the placement census)
  auto xst4 = [&](unsigned off, F4 v) __attribute__((always_inline)) { if (wt_) xbuf_st4<true>(xb, off, v); else xbuf_st4<false>(xb, off, v); };
  auto xst2 = [&](unsigned off, U2 v) __attribute__((always_inline)) { if (wt_) xbuf_st2<true>(xb, off, v); else xbuf_st2<false>(xb, off, v); };

  // ---- row-per-wave helpers (gathers, LayerNorm over whole rows, token assembly): lane l owns columns 4l .. 4l + 3 of a row
  auto st_row = [&](float* buf, int st, int row, F4 v) __attribute__((always_inline)) {       // -> split image, swizzled by the row
    unsigned h0, l0, h1, l1;
    split16_two(v.x, v.y, h0, l0);
    split16_two(v.z, v.w, h1, l1);
    unsigned* d = reinterpret_cast<unsigned*>(buf) + row * st + ((((lane >> 3) << 5) + ((lane & 7) << 1)) ^ (((row >> 2) & 3) << 2));
    *reinterpret_cast<U2*>(d) = U2{h0, h1};
    *reinterpret_cast<U2*>(d + 16) = U2{l0, l1};
  };
  auto ln_rows = [&](F4 (&v)[6], int nr, const float* gamma, const float* beta) __attribute__((always_inline)) {
    const F4 gm = ld4(gamma + lane * 4), bt = ld4(beta + lane * 4);
    float s[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = i < nr ? (v[i].x + v[i].y) + (v[i].z + v[i].w) : 0.f;
#if defined(CL_EXP) && (CL_EXP & 4)
    // measurement build (WRONG results, tools/loopbench only): no cross-lane reductions in the LayerNorms -- the upper bound of what row statistics published by the
    // producers of Y / the out-projection partials could buy
#define CL_SUM64(x) (x)
#else
#define CL_SUM64(x) sum64(x)
#endif
#pragma unroll
    for (int i = 0; i < 6; ++i) if (i < nr) s[i] = CL_SUM64(s[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < nr) {
        const float mean = s[i] * (1.0f / 256.0f);
        v[i] = F4{v[i].x - mean, v[i].y - mean, v[i].z - mean, v[i].w - mean};
        s[i] = (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) if (i < nr) s[i] = CL_SUM64(s[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < nr) {
        const float rs = rsqrtf(s[i] * (1.0f / 256.0f) + kLnEps);
        v[i] = F4{v[i].x * rs * gm.x + bt.x, v[i].y * rs * gm.y + bt.y, v[i].z * rs * gm.z + bt.z, v[i].w * rs * gm.w + bt.w};
      }
    }
  };
  auto f4add = [](F4 a, F4 b) { return F4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; };

  // token rows of a reverse step -> Xs (mld_denoiser.py:143-196): this wave's rows w + 8 i: token 0 = latent + pe[0] (both CFG halves of motion w),
  // token 1 = the step's time row, token 2 = the condition rows (unconditional, conditional)
  auto assemble = [&](int step) __attribute__((always_inline)) {
    const float* pe0 = sm_fin + 512;
    int sidx = s0 + wave;
    sidx = sidx < p.s_end ? sidx : p.s_end - 1;
    const F4 pe = ld4(pe0 + lane * 4), la = ld4(lats + wave * 256 + lane * 4), tt = ld4(p.T1 + (unsigned)step * 256u + lane * 4);
    const F4 tu = ld4(p.TP + (unsigned)sidx * 256u + lane * 4), tc = ld4(p.TP + (unsigned)(p.B + sidx) * 256u + lane * 4);
    const F4 x0 = f4add(la, pe);
    st_row(Xs, kClXs, wave, x0);
    st_row(Xs, kClXs, wave + 8, x0);
    st_row(Xs, kClXs, 16 + wave, tt);
    st_row(Xs, kClXs, 24 + wave, tt);
    st_row(Xs, kClXs, 32 + wave, tu);
    st_row(Xs, kClXs, 40 + wave, tc);
  };
  // a layer's small parameters (+ the bias of the skip linear behind it) -> LDS, double buffered (loop_fused.hpp prm_fetch / prm_store)
  F4 pf0, pf1;
  auto prm_fetch = [&](int layer) __attribute__((always_inline)) {
    const float* src = p.small + (unsigned)layer * (unsigned)kLsLayer;
    const int o0 = tid * 4, o1 = 2048 + o0;
    pf0 = ld4(src + o0);
    pf1 = o1 < kLsLayer ? ld4(src + o1) : F4{0.f, 0.f, 0.f, 0.f};
    if (o1 >= kLsLayer && o1 < kLsLayer + 256) {
      const int si = layer - nb;
      if (si >= 0 && layer + 1 < p.L) pf1 = ld4(p.small + (unsigned)p.L * (unsigned)kLsLayer + (unsigned)si * 256u + (unsigned)(o1 - kLsLayer));
    }
  };
  auto prm_store = [&](int buf) __attribute__((always_inline)) {
    float* dst = prm + buf * kLfPrmFloats;
    const int o0 = tid * 4, o1 = 2048 + o0;
    st4(dst + o0, pf0);
    if (o1 < kLfPrmFloats) st4(dst + o1, pf1);
  };

  // ---- prologue: latents, parameters of layer 0, the first step's rows, the ring; placement census when plain stores were asked for
  int step0 = 0;                                 // FROM: the first step this cluster runs
  [[maybe_unused]] int myf = 0;                  // FROM: first step of this wave's motion (s0 + wave; a ragged cluster's missing motions repeat the last real one)
  float myg = p.guidance;                        // FROM: guidance scale of this wave's motion, from its StartRow (global index: s_base included); else the launch's
  if constexpr (FROM) {
    const int c = tid >> 6, c4 = tid & 63;
    int s = s0 + c;
    s = s < p.s_end ? s : p.s_end - 1;
    const StartRow st = p.starts[s];             // (wave-uniform)
    F4 v = F4{0.f, 0.f, 0.f, 0.f};
    if (!(st.src && st.noised)) v = ld4(p.init_lat + (long long)s * 256 + c4 * 4);
    if (!st.src) {
      v = F4{v.x * p.init_sigma, v.y * p.init_sigma, v.z * p.init_sigma, v.w * p.init_sigma};
    } else {
      const F4 u = ld4_global(st.src + c4 * 4);
      const float ca = p.ddim[st.first_step * 4], cn = p.ddim[st.first_step * 4 + 1];      // add_noise at the first timestep that is run
      v = st.noised ? u : F4{ca * u.x + cn * v.x, ca * u.y + cn * v.y, ca * u.z + cn * v.z, ca * u.w + cn * v.w};
    }
    st4(lats + c * 256 + c4 * 4, v);
    myf = st.first_step;
    myg = st.guidance;
    step0 = p.n - 1;
    for (int k = 0; k < 8; ++k)
      if (s0 + k < p.s_end) { const int fk = p.starts[s0 + k].first_step; step0 = fk < step0 ? fk : step0; }
  } else {
    const int c = tid >> 6, c4 = tid & 63;
    int s = s0 + c;
    s = s < p.s_end ? s : p.s_end - 1;
    const F4 v = ld4(p.init_lat + (long long)s * 256 + c4 * 4);
    st4(lats + c * 256 + c4 * 4, F4{v.x * p.init_sigma, v.y * p.init_sigma, v.z * p.init_sigma, v.w * p.init_sigma});
  }
  prm_fetch(0);
  prm_store(0);
  if constexpr (CG == 4) { if (tid == 0) ctl[2] = 0u; }      // (wait_one of the 12-workgroup form)
  __syncthreads();
  assemble(step0);
#pragma unroll
  for (int j = 0; j < kClRing; ++j) gload(j);
  bool wt = true;
  if constexpr (!WT) {
    // every member posts 1 + its XCC id as its Z flag (Z epochs start above 16: see below); a cluster that spans XCDs keeps the write-through stores
    if (tid == 0) flag_store(flags + kFlagZ * kClFlagLine + member, 1u + xcc_id());
    if (!wait_flags(kFlagZ, all_mask, 1u)) { give_up(); return; }
    if (wave == 0) {
      const unsigned mine = 1u + xcc_id();
      const unsigned other = lane < kM ? flag_load(flags + kFlagZ * kClFlagLine + lane) : mine;
      const bool spans = wave_any(other != mine);
      if (lane == 0) { ctl[1] = spans ? 1u : 0u; if (spans && member == 0) flag_store(p.status + 1, 1u); }
    }
    __syncthreads();
    wt = ctl[1] != 0u;
  }
  wt_ = wt;
  __syncthreads();
  int pbuf = 0;
  const unsigned wg = blockIdx.x;
  // linear2 output + bias + residual (both added by its producer) of row `row`, this lane's 4 columns
  auto y_row = [&](unsigned par, int row) __attribute__((always_inline)) {
    return xbuf_ld4(xb, (kClY + par * 12288u + (unsigned)(row * 256 + lane * 4)) * 4u);
  };
  // norm1 output of the own token, row r, columns c0 .. c0 + 3 as the GEMMs saw it (high + low half of the As image): the residual of norm2
  auto h1_res = [&](int c0) __attribute__((always_inline)) {
    const int l4 = c0 >> 2;
    const unsigned* wq = reinterpret_cast<const unsigned*>(As) + r * kClXs + ((((l4 >> 3) << 5) + ((l4 & 7) << 1)) ^ swz4);
    const U2 h = *reinterpret_cast<const U2*>(wq), lo = *reinterpret_cast<const U2*>(wq + 16);
    return F4{f16_bits_value(h.x) + f16_bits_value(lo.x), f16_bits_value(h.x >> 16) + f16_bits_value(lo.x >> 16),
              f16_bits_value(h.y) + f16_bits_value(lo.y), f16_bits_value(h.y >> 16) + f16_bits_value(lo.y >> 16)};
  };

  for (int step = step0; step < p.n; ++step) {
    goff = wbase + (unsigned)(kClRing * kClFragFloats);
    for (int l = 0; l < p.L; ++l) {
      const float* sm = prm + pbuf * kLfPrmFloats;
      const unsigned epoch = (unsigned)((step - step0) * p.L + l) + 1u;
      const unsigned par = epoch & 1u;
      const unsigned own_mask = ((1u << CG) - 1u) << (CG * tk), ao_mask = 0xFu << (CG * tk);
      fresh();
      // ================= Ph1: Q (own token), K, V (all tokens) of head hc; 3-token attention for the 16 rows of token tk
      if (att) {
      if (wave < 4) {
        f32x4 q0 = zero4, q1 = zero4, k[3] = {zero4, zero4, zero4};
        F4 x[2][3][2];
#pragma unroll
        for (int t = 0; t < 3; ++t) frag(Xs, kClXs, 16 * t + r, 0, x[0][t]);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          if (kc + 1 < 8) {
#pragma unroll
            for (int t = 0; t < 3; ++t) frag(Xs, kClXs, 16 * t + r, kc + 1, x[(kc + 1) & 1][t]);
          }
          // the own token's fragments, selected without a dynamic register index
          F4 xo[2];
          xo[0] = tk == 0 ? x[kc & 1][0][0] : (tk == 1 ? x[kc & 1][1][0] : x[kc & 1][2][0]);
          xo[1] = tk == 0 ? x[kc & 1][0][1] : (tk == 1 ? x[kc & 1][1][1] : x[kc & 1][2][1]);
          mma1(2 * kc, xo, q0, q1);
          mma3(2 * kc + 1, x[kc & 1], k);
        }
        const F4 bq = ld4(sm + kLsInB + hc * 64 + wave * 16 + g * 4), bk = ld4(sm + kLsInB + 256 + hc * 64 + wave * 16 + g * 4);
        const float qv[4] = {q0[0] + q1[0] + bq.x, q0[1] + q1[1] + bq.y, q0[2] + q1[2] + bq.z, q0[3] + q1[3] + bq.w};
        const float bkv[4] = {bk.x, bk.y, bk.z, bk.w};
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          float sp = (qv[0] * (k[u][0] + bkv[0]) + qv[1] * (k[u][1] + bkv[1])) + (qv[2] * (k[u][2] + bkv[2]) + qv[3] * (k[u][3] + bkv[3]));
          sp = sum_groups(sp);
          if (g == 0) sc[(u * 16 + r) * 4 + wave] = sp;
        }
        __syncthreads();
      } else {
        const int w4 = wave - 4;
        f32x4 v[3] = {zero4, zero4, zero4};
        F4 x[2][3][2];
#pragma unroll
        for (int t = 0; t < 3; ++t) frag(Xs, kClXs, 16 * t + r, 0, x[0][t]);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          if (kc + 1 < 8) {
#pragma unroll
            for (int t = 0; t < 3; ++t) frag(Xs, kClXs, 16 * t + r, kc + 1, x[(kc + 1) & 1][t]);
          }
          mma3(kc, x[kc & 1], v);
        }
        const F4 bv = ld4(sm + kLsInB + 512 + hc * 64 + w4 * 16 + g * 4);
        const float bvv[4] = {bv.x, bv.y, bv.z, bv.w};
        __syncthreads();
        float a[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const F4 e = ld4(sc + (u * 16 + r) * 4);
          a[u] = ((e.x + e.y) + (e.z + e.w)) * (0.125f * 1.44269504088896340736f);      // 1 / sqrt(64), log2 domain
        }
        const float m = fmaxf(a[0], fmaxf(a[1], a[2]));
        const float e0 = fast_exp2(a[0] - m), e1 = fast_exp2(a[1] - m), e2 = fast_exp2(a[2] - m);
        const float inv = fast_rcp(e0 + e1 + e2);
        const float p0 = e0 * inv, p1 = e1 * inv, p2 = e2 * inv;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (p0 * (v[0][i] + bvv[i]) + p1 * (v[1][i] + bvv[i])) + p2 * (v[2][i] + bvv[i]);
        // attention output of head hc, row r, head dims 16 w4 + 4 g .. + 3 -> split image [16][64] in the As region (chunk w4 >> 1 of two)
        unsigned h0, l0, h1, l1;
        split16_two(o[0], o[1], h0, l0);
        split16_two(o[2], o[3], h1, l1);
        unsigned* wq = reinterpret_cast<unsigned*>(As) + r * kClAoS + (w4 >> 1) * 32 + (((w4 & 1) * 8 + g * 2) ^ swz4);
        *reinterpret_cast<U2*>(wq) = U2{h0, h1};
        *reinterpret_cast<U2*>(wq + 16) = U2{l0, l1};
      }
      __syncthreads();
      {
        // out-projection, split over K by HEAD: this member multiplies its head's 64 attention dims into all 256 output columns (this wave: 32 w .. + 31) and
        // publishes the raw partial; the four partials of a token are summed by everybody in E1 (one quarter of the weight bytes of a full out-projection per member)
        f32x4 a[2][2] = {{zero4, zero4}, {zero4, zero4}};
        F4 x[2][2];
        frag(As, kClAoS, r, 0, x[0]);
        frag(As, kClAoS, r, 1, x[1]);
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          mma1(2 * kc, x[kc], a[0][0], a[0][1], false);      // (16 or 8 fragments consumed so far in this phase: the ring slot is the same)
          mma1(2 * kc + 1, x[kc], a[1][0], a[1][1], false);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 pj = a[j][0] + a[j][1];
          xst4((kClPO + par * 49152u + (unsigned)(((tk * 4 + hc) * 16 + r) * 256 + wave * 32 + j * 16 + g * 4)) * 4u, F4{pj[0], pj[1], pj[2], pj[3]});
        }
      }
      CL_STAMP(0);
      publish(kFlagAO, epoch);
      refill();
      }
      CL_STAMP(1);
      fresh();
      // ================= E1: attention output of the token from its four members -> As
      if (!wait_flags(kFlagAO, ao_mask, epoch)) { give_up(); return; }
      CL_STAMP(2);
      {
        // rows w and w + 8 of the token: sum of the four partials (fixed order) + bias + residual (the layer input as the GEMMs saw it) -> norm1, in-wave
        F4 v[6];
        const F4 ob = ld4(sm + kLsOutB + lane * 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = wave + 8 * i;
          F4 acc4 = xbuf_ld4(xb, (kClPO + par * 49152u + (unsigned)(((tk * 4 + 0) * 16 + row) * 256 + lane * 4)) * 4u);
#pragma unroll
          for (int m = 1; m < 4; ++m) acc4 = f4add(acc4, xbuf_ld4(xb, (kClPO + par * 49152u + (unsigned)(((tk * 4 + m) * 16 + row) * 256 + lane * 4)) * 4u));
          const unsigned* wq = reinterpret_cast<const unsigned*>(Xs) + (16 * tk + row) * kClXs + ((((lane >> 3) << 5) + ((lane & 7) << 1)) ^ (((row >> 2) & 3) << 2));
          const U2 h = *reinterpret_cast<const U2*>(wq), lo = *reinterpret_cast<const U2*>(wq + 16);
          v[i] = F4{acc4.x + ob.x + (f16_bits_value(h.x) + f16_bits_value(lo.x)), acc4.y + ob.y + (f16_bits_value(h.x >> 16) + f16_bits_value(lo.x >> 16)),
                    acc4.z + ob.z + (f16_bits_value(h.y) + f16_bits_value(lo.y)), acc4.w + ob.w + (f16_bits_value(h.y >> 16) + f16_bits_value(lo.y >> 16))};
        }
        CL_STAMP(3);
        ln_rows(v, 2, sm + kLsN1W, sm + kLsN1B);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = wave + 8 * i;
          unsigned h0, l0, h1, l1;
          split16_two(v[i].x, v[i].y, h0, l0);
          split16_two(v[i].z, v[i].w, h1, l1);
          unsigned* d = reinterpret_cast<unsigned*>(As) + row * kClXs + ((((lane >> 3) << 5) + ((lane & 7) << 1)) ^ (((row >> 2) & 3) << 2));
          *reinterpret_cast<U2*>(d) = U2{h0, h1};
          *reinterpret_cast<U2*>(d + 16) = U2{l0, l1};
        }
      }
      __syncthreads();
      {
        F4 x[2][2];
        CL_STAMP(4);
        fresh();
        // linear1 + GELU
        if constexpr (CG == 4) {
        f32x4 h[2][2] = {{zero4, zero4}, {zero4, zero4}};
        frag(As, kClXs, r, 0, x[0]);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          if (kc + 1 < 8) frag(As, kClXs, r, kc + 1, x[(kc + 1) & 1]);
          mma1(2 * kc, x[kc & 1], h[0][0], h[0][1], 2 * kc + kClRing < 16);
          mma1(2 * kc + 1, x[kc & 1], h[1][0], h[1][1], 2 * kc + 1 + kClRing < 16);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const F4 b1 = ld4(sm + kLsL1B + hc * 256 + wave * 32 + j * 16 + g * 4);
          const float v0 = gelu_erf((h[j][0][0] + h[j][1][0]) + b1.x), v1 = gelu_erf((h[j][0][1] + h[j][1][1]) + b1.y);
          const float v2 = gelu_erf((h[j][0][2] + h[j][1][2]) + b1.z), v3 = gelu_erf((h[j][0][3] + h[j][1][3]) + b1.w);
          unsigned h0, l0, h1, l1;
          split16_two(v0, v1, h0, l0);
          split16_two(v2, v3, h1, l1);
          // the hidden activation travels as the (unswizzled) split image: row 16 tk + r, chunk 8 hc + w (32 hidden columns = 32 words), high words 8 j + 2 g, low + 16
          const unsigned wo = (kClH + par * 49152u + (unsigned)((16 * tk + r) * 1024 + (8 * hc + wave) * 32 + j * 8 + g * 2)) * 4u;
          xst2(wo, U2{h0, h1});
          xst2(wo + 64u, U2{l0, l1});
        }
        } else {
        // hidden columns 128 hc + 16 w .. + 15: one tile per wave, 8 fragments
        f32x4 ha = zero4, hb = zero4;
        frag(As, kClXs, r, 0, x[0]);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          if (kc + 1 < 8) frag(As, kClXs, r, kc + 1, x[(kc + 1) & 1]);
          mma1(kc, x[kc & 1], ha, hb, kc + kClRing < 8);
        }
        const F4 b1 = ld4(sm + kLsL1B + hc * 128 + wave * 16 + g * 4);
        const float v0 = gelu_erf((ha[0] + hb[0]) + b1.x), v1 = gelu_erf((ha[1] + hb[1]) + b1.y);
        const float v2 = gelu_erf((ha[2] + hb[2]) + b1.z), v3 = gelu_erf((ha[3] + hb[3]) + b1.w);
        unsigned h0, l0, h1, l1;
        split16_two(v0, v1, h0, l0);
        split16_two(v2, v3, h1, l1);
        // same image: chunk 4 hc + (w >> 1), tile w & 1 of the chunk
        const unsigned wo = (kClH + par * 49152u + (unsigned)((16 * tk + r) * 1024 + (4 * hc + (wave >> 1)) * 32 + (wave & 1) * 8 + g * 2)) * 4u;
        xst2(wo, U2{h0, h1});
        xst2(wo + 64u, U2{l0, l1});
        }
      }
      CL_STAMP(5);
      publish(kFlagH, epoch);
      refill();
      CL_STAMP(6);
      fresh();
      // ================= E2: the token's hidden activation (64 KB image) from its four members -> Xs region as [16][1032]
      if constexpr (CG == 4) {
        // every wave gathers the slice of ONE producer (wave w <- member (tk, w >> 1), rows 8 (w & 1) .. + 7) as soon as THAT member's flag is up: slices of early
        // producers are in LDS while the last one is still awaited, and there is no barrier between the poll and the loads
        const int prod = wave >> 1;
        wait_one(kFlagH, tk * CG + prod, epoch);
        CL_STAMP(7);
        F4 hv[8];
        int rows[8], uns[8];
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) {
          const int u = lane + 64 * k8;                 // 16-byte unit of the producer's slice: 8 rows x 64 units
          rows[k8] = 8 * (wave & 1) + (u >> 6);
          uns[k8] = 64 * prod + (u & 63);               // unit of the row's 256 (1024 words)
          hv[k8] = xbuf_ld4(xb, (kClH + par * 49152u + (unsigned)(16 * tk + rows[k8]) * 1024u) * 4u + (unsigned)uns[k8] * 16u);
        }
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8)
          st4(Xs + rows[k8] * kClHs + (((uns[k8] >> 2) << 4) + (((uns[k8] & 3) ^ ((rows[k8] >> 2) & 3)) << 2)), hv[k8]);
        __syncthreads();
        if (ctl[2] != 0u) { give_up(); return; }
      } else {
      if (!wait_flags(kFlagH, own_mask, epoch)) { give_up(); return; }
      CL_STAMP(7);
      {
        F4 hv[8];
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) {
          const int q = tid + 512 * k8;                 // 16-byte unit: row q >> 8, unit (q & 255) of the row's 1024 words
          hv[k8] = xbuf_ld4(xb, (kClH + par * 49152u + (unsigned)(16 * tk) * 1024u) * 4u + (unsigned)q * 16u);
        }
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) {
          const int q = tid + 512 * k8, row = q >> 8, un = q & 255;
          st4(Xs + row * kClHs + (((un >> 2) << 4) + (((un & 3) ^ ((row >> 2) & 3)) << 2)), hv[k8]);
        }
      }
      __syncthreads();
      }
      CL_STAMP(8);
      fresh();
      // ================= Ph3: linear2 for output columns 64 hc + 16 (w & 3) .. + 15, K half w >> 2; halves meet through LDS -> Y
      if constexpr (CG == 4) {
        f32x4 y0 = zero4, y1 = zero4;
        const int kh = wave >> 2;
        F4 x[2][2];
        frag(Xs, kClHs, r, 16 * kh, x[0]);
#pragma unroll
        for (int kc = 0; kc < 16; ++kc) {
          if (kc + 1 < 16) frag(Xs, kClHs, r, 16 * kh + kc + 1, x[(kc + 1) & 1]);
          mma1(kc, x[kc & 1], y0, y1, kc + kClRing < 16);
        }
        f32x4 y = y0 + y1;
#ifdef CL_TRACE
        asm volatile("" : "+v"(y));
        CL_STAMP(15);
#endif
        if (wave >= 4) *reinterpret_cast<f32x4*>(red2 + ((wave - 4) * 64 + lane) * 4) = y;
        __syncthreads();
        if (wave < 4) {
          y += *reinterpret_cast<const f32x4*>(red2 + (wave * 64 + lane) * 4);
          const F4 b2 = ld4(sm + kLsL2B + hc * 64 + wave * 16 + g * 4), rs = h1_res(hc * 64 + wave * 16 + g * 4);
          xst4((kClY + par * 12288u + (unsigned)((16 * tk + r) * 256 + hc * 64 + wave * 16 + g * 4)) * 4u,
               F4{(y[0] + b2.x) + rs.x, (y[1] + b2.y) + rs.y, (y[2] + b2.z) + rs.z, (y[3] + b2.w) + rs.w});
        }
      } else {
        // output columns 32 hc + 16 (w & 1) .. + 15, K quarter w >> 1 (8 fragments); the quarters meet through LDS in a fixed order
        f32x4 y0 = zero4, y1 = zero4;
        const int tile = wave & 1, kq = wave >> 1;
        F4 x[2][2];
        frag(Xs, kClHs, r, 8 * kq, x[0]);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          if (kc + 1 < 8) frag(Xs, kClHs, r, 8 * kq + kc + 1, x[(kc + 1) & 1]);
          mma1(kc, x[kc & 1], y0, y1, kc + kClRing < 8);
        }
        f32x4 y = y0 + y1;
#ifdef CL_TRACE
        asm volatile("" : "+v"(y));
        CL_STAMP(15);
#endif
        if (kq) *reinterpret_cast<f32x4*>(red2 + (((kq - 1) * 2 + tile) * 64 + lane) * 4) = y;
        __syncthreads();
        if (wave < 2) {
#pragma unroll
          for (int q = 0; q < 3; ++q) y += *reinterpret_cast<const f32x4*>(red2 + ((q * 2 + tile) * 64 + lane) * 4);
          const F4 b2 = ld4(sm + kLsL2B + hc * 32 + tile * 16 + g * 4), rs = h1_res(hc * 32 + tile * 16 + g * 4);
          xst4((kClY + par * 12288u + (unsigned)((16 * tk + r) * 256 + hc * 32 + tile * 16 + g * 4)) * 4u,
               F4{(y[0] + b2.x) + rs.x, (y[1] + b2.y) + rs.y, (y[2] + b2.z) + rs.z, (y[3] + b2.w) + rs.w});
        }
      }
      CL_STAMP(9);
      publish(kFlagY, epoch);
      refill();
      CL_STAMP(10);
      fresh();
      // ================= E3 and what follows the layer
      const bool last = l + 1 == p.L, skip_next = !last && l >= nb;
      prm_fetch(last ? 0 : l + 1);
      if (!wait_flags(kFlagY, all_mask, epoch)) { give_up(); return; }
      CL_STAMP(11);      // all twelve even where fewer rows are read (buffer-reuse invariant)
      if (!last && !skip_next) {
        // x' = norm2(y + h1) for all 48 rows -> Xs; input blocks park their own token's rows for the skip connection (cross_attention.py:48-52)
        F4 v[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = y_row(par, wave + 8 * i);
#ifdef CL_TRACE
        asm volatile("" : "+v"(v[0].x), "+v"(v[5].w));
        CL_STAMP(14);
#endif
        ln_rows(v, 6, sm + kLsN2W, sm + kLsN2B);
#pragma unroll
        for (int i = 0; i < 6; ++i) st_row(Xs, kClXs, wave + 8 * i, v[i]);
        if (l < nb) {
          float* pk = p.park + ((size_t)wg * nb + l) * (16 * 256);
#pragma unroll
          for (int i = 0; i < 6; ++i)
            if ((i >> 1) == tk) st4(pk + (unsigned)((wave + 8 * (i & 1)) * 256 + lane * 4), v[i]);
        }
        prm_store(pbuf ^ 1);
        __syncthreads();
      } else if (skip_next) {
        // norm2 of the token's own rows, then x = Linear(cat[x', skip]) for these 16 rows x 64 columns: K half 0 (x') on waves 0-3, half 1 (the parked rows) on waves 4-7
        const int si = l - nb;
        F4 v[6];
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i] = y_row(par, 16 * tk + wave + 8 * i);
        const float* pk = p.park + ((size_t)wg * nb + (nb - 1 - si)) * (16 * 256);
        const F4 s0v = ld4(pk + (unsigned)(wave * 256 + lane * 4)), s1v = ld4(pk + (unsigned)((wave + 8) * 256 + lane * 4));
        ln_rows(v, 2, sm + kLsN2W, sm + kLsN2B);
        st_row(Xs, kClXs, 16 * tk + wave, v[0]);
        st_row(Xs, kClXs, 16 * tk + wave + 8, v[1]);
        st_row(As, kClXs, wave, s0v);
        st_row(As, kClXs, wave + 8, s1v);
        __syncthreads();
        fresh();
        f32x4 z0 = zero4, z1 = zero4;
        const unsigned zepoch = 16u + (unsigned)((step - step0) * nb + si) + 1u, zpar = zepoch & 1u;
        if constexpr (CG == 4) {
        const float* abuf = wave < 4 ? Xs + 16 * tk * kClXs : As;
        F4 x[2][2];
        frag(abuf, kClXs, r, 0, x[0]);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          if (kc + 1 < 8) frag(abuf, kClXs, r, kc + 1, x[(kc + 1) & 1]);
          mma1(kc, x[kc & 1], z0, z1, kc + kClRing < 8);
        }
        f32x4 z = z0 + z1;
        if (wave >= 4) *reinterpret_cast<f32x4*>(red2 + ((wave - 4) * 64 + lane) * 4) = z;
        __syncthreads();
        if (wave < 4) {
          z += *reinterpret_cast<const f32x4*>(red2 + (wave * 64 + lane) * 4);
          const F4 sb = ld4(sm + kLsLayer + hc * 64 + wave * 16 + g * 4);
          xst4((kClZ + zpar * 12288u + (unsigned)((16 * tk + r) * 256 + hc * 64 + wave * 16 + g * 4)) * 4u, F4{z[0] + sb.x, z[1] + sb.y, z[2] + sb.z, z[3] + sb.w});
        }
        } else {
        // 32 columns per member: tile w & 1, K quarter w >> 1 of the 512 (quarters 0, 1: x', 2, 3: the parked rows), 4 fragments
        const int tile = wave & 1, kq = wave >> 1;
        const float* abuf = kq < 2 ? Xs + 16 * tk * kClXs : As;
        F4 x[2][2];
        frag(abuf, kClXs, r, 4 * (kq & 1), x[0]);
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
          if (kc + 1 < 4) frag(abuf, kClXs, r, 4 * (kq & 1) + kc + 1, x[(kc + 1) & 1]);
          mma1(kc, x[kc & 1], z0, z1, kc + kClRing < 4);
        }
        f32x4 z = z0 + z1;
        if (kq) *reinterpret_cast<f32x4*>(red2 + (((kq - 1) * 2 + tile) * 64 + lane) * 4) = z;
        __syncthreads();
        if (wave < 2) {
#pragma unroll
          for (int q = 0; q < 3; ++q) z += *reinterpret_cast<const f32x4*>(red2 + ((q * 2 + tile) * 64 + lane) * 4);
          const F4 sb = ld4(sm + kLsLayer + hc * 32 + tile * 16 + g * 4);
          xst4((kClZ + zpar * 12288u + (unsigned)((16 * tk + r) * 256 + hc * 32 + tile * 16 + g * 4)) * 4u, F4{z[0] + sb.x, z[1] + sb.y, z[2] + sb.z, z[3] + sb.w});
        }
        }
        publish(kFlagZ, zepoch);
      refill();
        fresh();
        if (!wait_flags(kFlagZ, all_mask, zepoch)) { give_up(); return; }
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = xbuf_ld4(xb, (kClZ + zpar * 12288u + (unsigned)((wave + 8 * i) * 256 + lane * 4)) * 4u);
#pragma unroll
        for (int i = 0; i < 6; ++i) st_row(Xs, kClXs, wave + 8 * i, v[i]);
        prm_store(pbuf ^ 1);
        __syncthreads();
      } else {
        // end of the step, every member for itself: norm2 + encoder.norm of the latent token's rows w (unconditional) and w + 8 (conditional) of motion w,
        // CFG (mld.py:339-342), DDIM (mld.py:345-346; eta = 0, or + sigma z: wave w owns motion s0 + w, lane the elements 4 lane .. + 3), the next step's rows
        F4 v[6];
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i] = y_row(par, wave + 8 * i);
        ln_rows(v, 2, sm + kLsN2W, sm + kLsN2B);
        ln_rows(v, 2, sm_fin, sm_fin + 256);
        const float sat = p.ddim[step * 4], s1mat = p.ddim[step * 4 + 1], sap = p.ddim[step * 4 + 2], s1map = p.ddim[step * 4 + 3];
        float* lp = lats + wave * 256 + lane * 4;
        const F4 xt = ld4(lp);
        const float eu[4] = {v[0].x, v[0].y, v[0].z, v[0].w}, ec[4] = {v[1].x, v[1].y, v[1].z, v[1].w}, xtv[4] = {xt.x, xt.y, xt.z, xt.w};
        float nv[4];
        if constexpr (ETA) {
          // x' = sqrt_ap x0 + sqrt(1 - ab_p - sigma^2) eps + sigma z (a ragged cluster's missing motions hold no key: z = 0 there)
          const float ce = p.eta[step * 2], sg = p.eta[step * 2 + 1];
          float z[4] = {0.f, 0.f, 0.f, 0.f};
          if (s0 + wave < p.s_end) latent_noise4(p.keys[s0 + wave], (unsigned)step, lane, z);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float eps = eu[i] + myg * (ec[i] - eu[i]);
            const float x0 = (xtv[i] - s1mat * eps) / sat;
            nv[i] = sap * x0 + ce * eps;
            nv[i] += sg * z[i];
          }
        } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float eps = eu[i] + myg * (ec[i] - eu[i]);
          const float x0 = (xtv[i] - s1mat * eps) / sat;
          nv[i] = sap * x0 + s1map * eps;
        }
        }
        bool hold = false;
        if constexpr (FROM) {                      // a motion that has not started yet keeps its latent: a select on the stored value (wave-uniform)
          hold = step < myf;
#pragma unroll
          for (int i = 0; i < 4; ++i) nv[i] = hold ? xtv[i] : nv[i];
        }
        st4(lp, F4{nv[0], nv[1], nv[2], nv[3]});
        // the step's prev_sample to the motion's trajectory row: member 0 (as with p.lat), wave w = motion s0 + w (wave-uniform test; no barrier, no LDS)
        if (member == 0 && p.traj && s0 + wave < p.s_end && !hold) {
          const TrajRow tr = p.traj[s0 + wave];
          if (tr.row0) st4_global(tr.row0 + (long long)step * tr.step_stride + lane * 4, F4{nv[0], nv[1], nv[2], nv[3]});
        }
        prm_store(pbuf ^ 1);
        if (step + 1 < p.n) assemble(step + 1);      // (reads this wave's own latent row only)
        __syncthreads();
      }
      CL_STAMP(12);
      pbuf ^= 1;
    }
  }
#ifdef CL_TRACE
  if (p.trace && lane == 0) {
    unsigned long long* o = p.trace + ((size_t)blockIdx.x * 8 + wave) * 16;
    for (int k = 0; k < 16; ++k) o[k] = ph[k];
  }
#endif
  if (member == 0) {
    const int c = tid >> 6, c4 = tid & 63;
    if (s0 + c < p.s_end) st4(p.lat + (long long)(s0 + c) * 256 + c4 * 4, ld4(lats + c * 256 + c4 * 4));
  }
  // Every polled word goes back to zero before the launch ends: a member that is past its last wait counts itself in word 28 of the Z line; the
  // last arrival polls nothing any more and neither does anybody else, so it clears the cluster's flag words.  clear_cluster_flags_kernel in front of
  // the launch (Guideline 16 "Re-initialise every call") does it again.
  __syncthreads();
  if (tid == 0) {
#if defined(MLDHIP_SIM)
    const unsigned prev = flags[kFlagZ * kClFlagLine + 28]++;
#else
    const unsigned prev = __hip_atomic_fetch_add(flags + kFlagZ * kClFlagLine + 28, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    if (prev == (unsigned)kM - 1u)
      for (int i = 0; i < kClFlagWords; ++i) flag_store(flags + i, 0u);
  }
