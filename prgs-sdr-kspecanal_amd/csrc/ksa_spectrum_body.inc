// The body of spectrum_kernel (ksa_kernels.hpp includes this text inside the kernel: once in spectrum_kernel and, in the experiments
// build, once more in spectrum_plain_kernel).  Expects in scope: the template parameters N, FMT, RM, CM, the kernel argument p and
// PK, the arithmetic of the butterflies (true: Packed, false: Scalar; ksa_fft.hpp).  An included file and not a function: called as
// an inlined function the same text compiles to different code in every instantiation (other register numbers, other spills).
  static_assert(RM == 0 || Plan<N>::S == 1, "sample reuse needs one transform per workgroup");
  using P = Plan<N>;
  using AR = std::conditional_t<PK, Packed, Scalar>;
  constexpr int L = P::L, T = P::T, S = P::S, M = P::M, R0 = P::R0, B0 = P::B0, NPAD = P::NPAD;
  constexpr int SB = fmt_bytes(FMT);  // bytes per IQ sample
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float2* const tw_lds = lds + S * NPAD;

  const int tid = threadIdx.x;
  const int slot = S == 1 ? 0 : tid / L;   // S == 1: constant, keeps window indices wave-uniform (scalar loads)
  const int l = tid - slot * L;
  float2* const my = lds + slot * NPAD;

  // ---- per-thread constants: window taps (VGPRs or LDS) and last-pass twiddles (VGPRs) --------
  constexpr bool WIN_LDS = Tune<N>::WIN_LDS;
  float* const win_lds = reinterpret_cast<float*>(tw_lds + P::MID);   // [4][L][4] floats, shared by the slots
  float win[16];
  if constexpr (WIN_LDS) {
    for (int i = tid; i < N; i += T) {       // tap of sample n = l' + L*q lives at ((q>>2)*L + l')*4 + (q&3)
      const int q = i / L, ll = i - q * L;
      win_lds[((q >> 2) * L + ll) * 4 + (q & 3)] = p.window[i] * tap_scale<FMT>(p);
    }
  } else if constexpr (!Tune<N>::WIN_GLOBAL) {
#pragma unroll
    for (int q = 0; q < 16; ++q) win[q] = p.window[l + L * q] * tap_scale<FMT>(p);
  }
  // last pass: k = l.  FUSED: the 15 folded twiddles of dft16_fused (rows of the [15][N/16] table);
  // otherwise rows t = 1,2,3,4,8,12 of the plain w^t table for dft16_tw.
  constexpr bool FUSED = Tune<N>::FUSED, FUSED_LAST = Tune<N>::FUSED_LAST;
  float2 twl[FUSED_LAST ? 15 : 6];
  if constexpr (M >= 2) {
    if constexpr (FUSED_LAST) {
#pragma unroll
      for (int e = 0; e < 15; ++e) twl[e] = p.tw_last[e * P::P_LAST + l];
    } else {
      constexpr int rows[6] = {0, 1, 2, 3, 7, 11};
#pragma unroll
      for (int e = 0; e < 6; ++e) twl[e] = p.tw_last[rows[e] * P::P_LAST + l];
    }
  }
  // M == 3: the 15 folded middle-pass twiddles of a thread (they depend on l mod R0 only) live in VGPRs as well -- the
  // transposed exchange layout freed ~30 registers (136 instead of 168 at N = 4096), which is exactly what they need.
  // Measured at config 2 on one box: re-read from LDS per window 5.76 ms, in VGPRs 5.62 ms, with the prefetch below 5.51 ms.
  // (M > 3, experiments builds only, keeps the tables of its middle passes in LDS.)
#ifndef KSA_TWM_REGS
#define KSA_TWM_REGS 1
#endif
  constexpr bool TWM_REGS = KSA_TWM_REGS && M == 3 && FUSED;
  float2 twm[15];
  if constexpr (TWM_REGS) {
#pragma unroll
    for (int e = 0; e < 15; ++e) twm[e] = p.tw_mid[e * R0 + (l & (R0 - 1))];
  } else if constexpr (P::MID > 0) {
    for (int i = tid; i < P::MID; i += T) tw_lds[i] = p.tw_mid[i];
  }

  if constexpr (WIN_LDS) __syncthreads();   // taps are read before the first exchange barrier

  const int nm1 = p.nwin - 1;
  const int NP = p.parts > 1 ? p.parts : 1;   // window split: latency mode for batches smaller than the GPU

  // Raw IQ of one window per thread: 16 samples l + L*q, loaded at the top of the window (8 B/lane, 512 B per
  // wave-instruction).  The buffer descriptor is built from scalars only (a per-lane descriptor makes hipcc wrap
  // every load in a readfirstlane "waterfall" loop) and spans exactly this frame: every load is range-checked
  // by the hardware.  Prefetching the next window into a second register set was measured and dropped
  // (spills: 104 -> 165 M FFT/s without it at the 0.1 hop; 2.5 -> 1.6 ms with sample reuse).
  typedef typename RawOf<FMT>::type raw_t;
  raw_t raw[16];
  const int start0 = p.starts[0];
  auto issue_loads = [&](int fr, int k, int q0, auto rotc) {
    constexpr int ROT = decltype(rotc)::value;   // ping-pong form: sample q lands in raw[(q + ROT) & 15]
    const char* fbase = reinterpret_cast<const char*>(p.iq) + (long long)fr * p.frame_stride * SB;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(fbase), 0, p.frame_len * SB, 0x00020000);
    // reuse path: hops are constant (RM*L samples), so the start is arithmetic -- no dependent scalar load
    const int start = RM > 0 ? start0 + k * (RM * L) : p.starts[k];
    const int voff = (start + l) * SB;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (q < q0) continue;
#ifdef KSA_ABL_NOLOAD   // timing-only ablation build: wrong results by construction
      if constexpr (FMT == FMT_C64) { raw[(q + ROT) & 15].x = voff + q; raw[(q + ROT) & 15].y = voff * q; }
      else raw[(q + ROT) & 15] = voff + q;
#else
#ifndef KSA_LOAD_AUX
#define KSA_LOAD_AUX 0   // cache policy of the IQ loads (experiments: 2 = nt)
#endif
      if constexpr (FMT == FMT_C64) raw[(q + ROT) & 15] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, L * q * SB, KSA_LOAD_AUX);
      else if constexpr (FMT == FMT_S16) raw[(q + ROT) & 15] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, L * q * SB, 0);
      else raw[(q + ROT) & 15] = __builtin_amdgcn_raw_buffer_load_b16(rsrc, voff, L * q * SB, 0);
#endif
    }
  };
  auto shift_raw = [&]() {
#pragma unroll
    for (int q = 0; q + RM < 16; ++q) raw[q] = raw[q + RM];
  };

#ifdef KSA_STAMPS
  unsigned long long seg[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_last;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_last)::"memory");
#endif
#ifndef KSA_PF
#define KSA_PF 1   // reuse path: the RM new samples of window k+1 are requested while window k is transformed.  Fits since the
                   // transposed exchange layout of round 4: alone 155 VGPRs and no spill; together with the middle twiddles in
                   // VGPRs (TWM_REGS) the N = 4096 reuse kernels sit at the 168-VGPR cap; what the rolled loop spills (2-8 registers:
                   // 75 % overlap, MAX / MIN folds) is stored before the window loop and reloaded in the output stage -- never
                   // inside the loop (tests/test_isa_regression.py holds the compiler to that).  +1.9 % at config 2, +0.6 % at 75 % overlap,
                   // +1..3 % at N = 2048; N = 1024 would spill 6-8 registers and large batches run the pair kernel there anyway
#endif
  // (requesting the first window of the workgroup's NEXT frame before this frame's output stage, with LDS-only barriers
  //  around the staging stores so that the loads stay in flight, measured 2.5 % SLOWER at config 2: profiles/r04_ab_prefetch_twiddles.txt)
  constexpr bool PF = KSA_PF && RM > 0 && N >= 2048;
  // Ping-pong form of the 50 %-overlap kernels of N = 4096 (round 5): at RM = 8 a window's new half is the next window's old half, so
  // instead of moving registers every window (shift the carried half down, copy the prefetched half in: 24 v_mov_b64 per window in
  // the rolled loop) the loop holds TWO windows and the halves of raw[] swap roles with the window's parity (ksa_window_body.inc is
  // included twice, PAR = 0 / 1: sample q sits in raw[(q + 8*PAR) & 15], the prefetch lands in the half that has just been converted).
  // 8 moves per window are left, the AVG kernel spills nothing any more (8 registers in the rolled form), and since every VALU
  // instruction of this kernel costs its full issue time (profiles/r05_sensitivity_c2.txt) that is time: config 2 +1.8 %, uint8 input
  // +3..5 % (profiles/r05_ab_pp.txt).  The body is an included file and not a lambda on purpose: as a generic lambda the same code made
  // hipcc spill 9-12 registers in kernels that do not use it (N = 2048: 78 with it).
#ifndef KSA_PP
#define KSA_PP 1
#endif
  constexpr bool PP = KSA_PP && PF && RM == 8 && N == 4096;
  // (General path, RM == 0: letting the raw-sample registers take the NEXT round's 16 loads as soon as a round has converted
  //  them was measured at N = 64, round 5: 168 instead of 121 VGPRs = three instead of four waves per SIMD, config 4 14.9 vs
  //  17.7 G FFT/s (-16 %; uint8 -15 %); held to 128 VGPRs the same code spills 98-110 registers, with the 6-twiddle last pass
  //  as well: profiles/r05_ab_pf0.txt.  Removed.)
  // Which units (frames, or (frame, part) in window-split mode) a workgroup transforms.  The three workgroups of a CU do not
  // run equally fast -- the SIMDs issue oldest wave first, so under an equal split the first workgroup of every CU ends at 64 %
  // of the launch, the second at 80 %, and the CU finishes its share at two and then one wave per SIMD
  // (profiles/ticket_skew.txt) -- so units are handed out on demand: the first is blockIdx.x, every later one is
  // gridDim.x + a ticket drawn from p.tickets (zero at the launch).  The ticket is requested by one lane at the start of the
  // output stage and consumed behind it (ticket_next: one LDS word, one barrier per unit): nothing of it is live inside the window loop.
  // The word is the last one of the transform's data region, which the output stage does not touch (its rows fill the front
  // half) and the next unit stores to only behind its first exchange barrier.  One unit per ticket, so only where a unit is
  // long (S == 1, and the host hands the counter over only where a unit's windows make the draws rare); a unit's results are a
  // function of its index alone, whoever computes it.
  constexpr bool TICKETS = S == 1;
  static_assert(!TICKETS || NPAD > N, "the ticket word lies behind the output stage's two planes of N floats");
  const int units = p.nframes * NP;
  unsigned* const next_unit = reinterpret_cast<unsigned*>(lds + S * NPAD) - 1;
  KSA_SKEW_BEGIN();
  for (int vf = blockIdx.x; vf < units;) {
    KSA_SKEW_UNIT();
    const int frame = vf / NP, part = vf - frame * NP;
    // this workgroup's contiguous share of the frame's windows (contiguous keeps the sample reuse valid)
    const int k_lo = (int)((long long)p.nwin * part / NP), k_hi = (int)((long long)p.nwin * (part + 1) / NP);
    const int rounds = (k_hi - k_lo + S - 1) / S;
    float acc[16];
    const float init = p.cumu == CUMU_MIN ? __builtin_inff() : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = init;

    if constexpr (PP) {
      for (int rd0 = 0; rd0 < rounds; rd0 += 2) {
        {
          const int rd = rd0;
          constexpr int PAR = 0;
#include "ksa_window_body.inc"
        }
        if (rd0 + 1 < rounds) {
          const int rd = rd0 + 1;
          constexpr int PAR = 1;
#include "ksa_window_body.inc"
        }
      }
    } else {
      for (int rd = 0; rd < rounds; ++rd) {
        constexpr int PAR = 0;
#include "ksa_window_body.inc"
      }
    }

    // ---- combine the slots, scale, fftshift, dB, waterfall row ------------------------------
    // register position i of thread (slot,l) is bin l + L*perm16(i)   (M == 1: N == 16, L == 1).
    // The fold result goes through LDS once per frame so that the (rolled, branchy) output stage
    // does not share registers with the transform loop.
    float* const red = reinterpret_cast<float*>(lds);  // [S][N] floats, inside the data region
    __syncthreads();
    KSA_STAMP(9);    // output stage, part 1: the barrier behind the last window (slowest wave, outstanding loads)
    unsigned ticket = 0;
    if constexpr (TICKETS) {
      if (p.tickets && tid == 0) ticket = __hip_atomic_fetch_add(p.tickets, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) red[slot * RedStride<N, S>::value + l + L * perm<16>(i)] = acc[i];
    __syncthreads();
    KSA_STAMP(10);   // part 2: fold -> LDS staging + barrier
#ifdef KSA_ABL_NOFIN   // timing-only ablation build: one store per thread keeps the fold alive
    if (red[tid] == 123.456f) p.out[tid] = red[tid];
#else
    if (NP == 1) {
      finish_frame<N, T, S, CM>(p, red, frame, tid);
    } else {
      // partial fold of this share, slots combined, natural bin order; combine_parts_kernel finishes the frame
      float4* const dst = reinterpret_cast<float4*>(p.part_out + (long long)vf * N);
      const float4* red4 = reinterpret_cast<const float4*>(red);
      for (int q = tid; q < N / 4; q += T) {
        float4 r = red4[q];
        if constexpr (S > 1) {
          for (int s2 = 1; s2 < S; ++s2) {
            const float4 x = red4[s2 * (RedStride<N, S>::value / 4) + q];
            if (CM == CUMU_PSD || p.cumu == CUMU_AVG) { r.x += x.x; r.y += x.y; r.z += x.z; r.w += x.w; }
            else if (p.cumu == CUMU_MAX) { r.x = nan_max(r.x, x.x); r.y = nan_max(r.y, x.y); r.z = nan_max(r.z, x.z); r.w = nan_max(r.w, x.w); }
            else { r.x = nan_min(r.x, x.x); r.y = nan_min(r.y, x.y); r.z = nan_min(r.z, x.z); r.w = nan_min(r.w, x.w); }
          }
        }
        dst[q] = r;
      }
    }
#endif
    KSA_STAMP(8);
    if (TICKETS && p.tickets) vf = ticket_next<T>(ticket, next_unit);
    else vf += gridDim.x;
  }
  KSA_SKEW_END();
#ifdef KSA_STAMPS
  if (p.dbg && (tid & 63) == 0) {
    for (int i = 0; i < 12; ++i) p.dbg[((long long)blockIdx.x * (T / 64) + tid / 64) * 12 + i] = seg[i];
  }
#endif
