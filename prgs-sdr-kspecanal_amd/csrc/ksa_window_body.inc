// One window of spectrum_kernel's loop (ksa_kernels.hpp includes this text inside the kernel: once in the rolled loop, twice --
// with PAR = 0 and PAR = 1 -- in the ping-pong form of the 50 %-overlap kernels of N = 4096).  Expects in scope: rd, PAR, the
// arithmetic policy AR (ksa_fft.hpp) and everything the kernel has set up in front of its window loop.  Sample q of the window sits in raw[(q + 8*PAR) & 15].
      const int k = k_lo + (S == 1 ? rd : rd * S + slot);   // wave-uniform when one transform fills the workgroup
      const bool active = S == 1 || k < k_hi;
      float2 v[16];
      float wpos[16];   // WIN_FUSED: the taps in the register order of v
      if (PF) { if (rd == 0) issue_loads(frame, k, 0, std::integral_constant<int, 0>{}); }
      else if (active) issue_loads(frame, k, (RM > 0 && rd > 0) ? 16 - RM : 0, std::integral_constant<int, 0>{});
      if (active) {
        if constexpr (!WIN_LDS && Tune<N>::WIN_GLOBAL) {
          // scalar descriptor + scalar offsets: no per-load address VGPRs
          const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.window), 0, N * 4, 0x00020000);
#pragma unroll
          for (int q = 0; q < 16; ++q)
            win[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrsrc, l * 4, L * q * 4, 0)) * tap_scale<FMT>(p);
        }
        if constexpr (WIN_LDS) {
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const float4 w4 = reinterpret_cast<const float4*>(win_lds)[q4 * L + l];
            win[4 * q4 + 0] = w4.x; win[4 * q4 + 1] = w4.y; win[4 * q4 + 2] = w4.z; win[4 * q4 + 3] = w4.w;
          }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int pos = (q % B0) * R0 + (q / B0);
          float2 x;
          if constexpr (FMT == FMT_C64) {
            // (scalar copies first: __builtin_bit_cast on a vector element reads element 0 twice)
            const unsigned xr = raw[(q + 8 * PAR) & 15].x, xi = raw[(q + 8 * PAR) & 15].y;
            x = make_float2(__uint_as_float(xr), __uint_as_float(xi));
          } else if constexpr (FMT == FMT_S8 || FMT == FMT_S16) {
            x = unpack_signed<FMT>(raw[(q + 8 * PAR) & 15]);   // b * w, taps pre-multiplied by 2^-7 / 2^-15
          } else {
            const unsigned short b = raw[(q + 8 * PAR) & 15];   // (b - offset)/scale * w, taps pre-divided by the scale
            x = make_float2((float)(b & 0xff) - p.u8_offset, (float)(b >> 8) - p.u8_offset);
          }
          if constexpr (Tune<N>::WIN_FUSED) { v[pos] = x; wpos[pos] = win[q]; }
          else v[pos] = make_float2(x.x * win[q], x.y * win[q]);
        }
        // int8 / int16, rolled sample-reuse loop: a scheduling fence behind the unpack.  Without it hipcc spreads the 32 conversions
        // over the first pass, and spectrum_kernel<1024, int16, RM = 4, MIN> ends at the 168-VGPR cap with 5 spilled registers (161
        // and none with it).  Not on the general path: there the fence costs the N = 16 kernels a wave per SIMD (82 VGPRs).
        if constexpr ((FMT == FMT_S8 || FMT == FMT_S16) && RM > 0 && !PP) __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (PP) {
        // ping-pong: the window's old half is dead, its registers take the next window's new half, and the halves swap roles
        // with the window's parity instead of being moved
        issue_loads(frame, k + 1 < k_hi ? k + 1 : k, 8, std::integral_constant<int, 8 * (1 - PAR)>{});
      } else if (RM > 0) {
        shift_raw();   // the next round of this frame loads only its RM new samples
        // prefetch: the freed registers take window k+1's new samples now (unconditionally: after the frame's last
        // window the same samples are simply requested again), in flight under the three passes
        if (PF) issue_loads(frame, k + 1 < k_hi ? k + 1 : k, 16 - RM, std::integral_constant<int, 0>{});
      }
      KSA_STAMP(0);
      if (active) {
        if constexpr (Tune<N>::WIN_FUSED) dft_first_win<R0, AR>(v, wpos);
        else dft_first<R0>(v);
      }
      KSA_STAMP(1);
      if constexpr (Tune<N>::QUAD_XCHG) {
        // N = 64 = 4 * 16: butterfly i = l + 4b wrote output t to position 4l + 16b + t, the last pass reads
        // l' + 4t': register 4b + j of lane l' must hold what register 4b + l' of lane j holds -- a 4x4 transpose
        // inside the quad for every b, real and imaginary parts alike.  (The lanes of a quad share one slot, so
        // `active` is uniform over the quad.)
        static_assert(!Tune<N>::QUAD_XCHG || (L == 4 && R0 == 4 && M == 2), "quad exchange: N = 64 only");
        const bool odd1 = l & 1, odd2 = l & 2;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          quad_transpose4(v[4 * b].x, v[4 * b + 1].x, v[4 * b + 2].x, v[4 * b + 3].x, odd1, odd2);
          quad_transpose4(v[4 * b].y, v[4 * b + 1].y, v[4 * b + 2].y, v[4 * b + 3].y, odd1, odd2);
        }
        if (active) {
          if constexpr (FUSED_LAST) dft16_fused<AR>(v, reinterpret_cast<const float2(&)[15]>(twl));
          else dft16_tw(v, twl[0], twl[1], twl[2], twl[3], twl[4], twl[5]);
        }
      } else if constexpr (M >= 2) {
        KSA_SYNC();  // previous round's / frame's LDS reads are done
        KSA_STAMP(2);
        if (active) {
#pragma unroll
          for (int b = 0; b < B0; ++b) {
            const int i = l + b * L;  // butterfly index, p = 1
#pragma unroll
            for (int t = 0; t < R0; ++t) {
              if constexpr (P::XLAYOUT) KSA_LDS_ST(my[perm<R0>(t) * P::ST1 + i], v[b * R0 + t]);   // transposed: [output][butterfly]
              else KSA_LDS_ST(my[padi(i * R0 + perm<R0>(t))], v[b * R0 + t]);
            }
          }
        }
        KSA_SYNC();
        KSA_STAMP(3);
        int pp = R0;       // product of the radices already applied
        int tw_off = 0;
#pragma unroll
        for (int s = 1; s < M; ++s) {
          if (active) {
            if constexpr (!P::XLAYOUT) {
#pragma unroll
              for (int t = 0; t < 16; ++t) KSA_LDS_LD(v[t], my[padi(l + L * t)]);
            } else if (s == 1) {
              // exchange 1, element l + L*t = output l % R0 of first-pass butterfly l / R0 + (L/R0)*t
              const float2* const src = my + (l % R0) * P::ST1 + l / R0;
#pragma unroll
              for (int t = 0; t < 16; ++t) KSA_LDS_LD(v[t], src[(L / R0) * t]);
            } else {
              // exchange 2, element l + L*t in natural order with K2 pads per 2^SH2 (L = 2^SH2)
              const float2* const src = my + l + P::K2 * (l >> P::SH2);
#pragma unroll
              for (int t = 0; t < 16; ++t) KSA_LDS_LD(v[t], src[(L + P::K2) * t]);
            }
            if (s < M - 1) {
              const float2* tw = tw_lds + tw_off + (l & (pp - 1));
              if constexpr (TWM_REGS) {
                dft16_fused<AR>(v, reinterpret_cast<const float2(&)[15]>(twm));
              } else if constexpr (FUSED) {
                float2 tm[15];
#pragma unroll
                for (int e = 0; e < 15; ++e) tm[e] = tw[e * pp];
                dft16_fused<AR>(v, tm);
              } else {
                dft16_tw(v, tw[0], tw[pp], tw[2 * pp], tw[3 * pp], tw[7 * pp], tw[11 * pp]);
              }
            } else {
              if constexpr (FUSED_LAST) dft16_fused<AR>(v, reinterpret_cast<const float2(&)[15]>(twl));
              else dft16_tw(v, twl[0], twl[1], twl[2], twl[3], twl[4], twl[5]);
            }
          }
          KSA_STAMP(s < M - 1 ? 4 : 6);
          if (s < M - 1) {
            KSA_SYNC();
            if (active) {
              const int kk = l & (pp - 1);
              const int j = (l - kk) * 16 + kk;
              if constexpr (P::XLAYOUT) {       // (M == 3: pp == R0; every element of this butterfly shares j >> SH2 = l / pp)
                float2* const dst = my + j + P::K2 * (l >> ilog2(R0));
#pragma unroll
                for (int t = 0; t < 16; ++t) KSA_LDS_ST(dst[perm<16>(t) * R0], v[t]);
              } else {
#pragma unroll
                for (int t = 0; t < 16; ++t) KSA_LDS_ST(my[padi(j + perm<16>(t) * pp)], v[t]);
              }
            }
            KSA_SYNC();
            KSA_STAMP(5);
            tw_off += 15 * pp;
            pp *= 16;
          }
        }
      }
      // ---- |X| and the fold over this block's windows (K:391-395) ----------------------------
      if (active) {
        const int cm = CM == 0 ? p.cumu : CM;   // CM != 0: the fold mode is a compile-time constant
        if constexpr (CM == CUMU_PSD) {
          // Welch: the sum of |X|^2 over the windows, two FMAs per bin -- no square root, no per-window weight
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = fmaf(v[i].x, v[i].x, fmaf(v[i].y, v[i].y, acc[i]));
        } else if (cm == CUMU_AVG) {
          // closed form of the (a+x)/2 recursion: weight 2^-(n-k+1), first window 2^-n
          const int e = k == 0 ? nm1 : nm1 - k + 1;
          const float w = ldexpf(1.0f, -e);
#pragma unroll
          for (int i = 0; i < 16; ++i)
            acc[i] = fmaf(w, __builtin_amdgcn_sqrtf(fmaf(v[i].x, v[i].x, v[i].y * v[i].y)), acc[i]);
        } else if (cm == CUMU_MAX) {      // np.max / np.min of K:141-143: a NaN window keeps the bin NaN
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = nan_max_nonneg(acc[i], fmaf(v[i].x, v[i].x, v[i].y * v[i].y));
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = nan_min(acc[i], fmaf(v[i].x, v[i].x, v[i].y * v[i].y));
        }
      }
      KSA_STAMP(7);
