// Body of mixed_radix_kernel / mixed_radix_psd_kernel (ksa_kernels_mr.hpp includes this text inside both kernels, as
// ksa_window_body.inc is included by spectrum_kernel).  Expects in scope: FMT, p, plan and CM -- CUMU_PSD, or 0 = the
// AVG / MAX / MIN fold decided at run time from p.cumu.
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  constexpr int SB = fmt_bytes(FMT);   // bytes per IQ sample
  constexpr int NBL = MrNb<4>::value;          // butterflies per thread of the last (radix-4) pass
  const int T = blockDim.x;
  const int nm1 = p.nwin - 1;
  const auto lrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(plan.tw + plan.tw_off[plan.npass - 1]), 0, 3 * (plan.n / 4) * 8, 0x00020000);
  for (int frame = blockIdx.x; frame < p.nframes; frame += gridDim.x) {
    const char* const fbase = reinterpret_cast<const char*>(p.iq) + (long long)frame * p.frame_stride * SB;
    // acc[i][r]: bin j + r*N/4 of butterfly j = tid + i*T
    float acc[NBL][4];
    const float init = p.cumu == CUMU_MIN ? __builtin_inff() : 0.0f;
#pragma unroll
    for (int i = 0; i < NBL; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][r] = init;
    for (int k = 0; k < p.nwin; ++k) {
      int tid = threadIdx.x, n = plan.n;
      mr_opaque(tid, n);
      const int q4 = n / 4;
      mr_first_any<FMT>(plan.radix[0], p, fbase, p.starts[k], lds, n, tid, T);
      int ns = plan.radix[0];
      for (int s = 1; s < plan.npass - 1; ++s) {
        mr_mid_any(plan.radix[s], lds, plan.tw + plan.tw_off[s], n, ns, tid, T);
        ns *= plan.radix[s];
      }
      // last pass, radix 4 with ns = N/4: butterfly j reads j + r*N/4 and keeps its outputs (bins j + r*N/4) in registers
      // ---- |X| and the fold over this block's windows (K:391-395), as ksa_window_body.inc
      const int e = k == 0 ? nm1 : nm1 - k + 1;
      const float wk = ldexpf(1.0f, -e);
#pragma unroll
      for (int i = 0; i < NBL; ++i) {
        const int j = tid + i * T;
        if (j < q4) {
          float2 v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = lds[j + r * q4];
#pragma unroll
          for (int r = 1; r < 4; ++r) {
            const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(lrsrc, j * 8, (r - 1) * q4 * 8, 0);
            const unsigned tx = t.x, ty = t.y;
            v[r] = cmul(v[r], make_float2(__uint_as_float(tx), __uint_as_float(ty)));
          }
          mr_dft<4>(v);
          if constexpr (CM == CUMU_PSD) {    // Welch: the sum of |X|^2
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = fmaf(v[r].x, v[r].x, fmaf(v[r].y, v[r].y, acc[i][r]));
          } else if (p.cumu == CUMU_AVG) {       // closed form of the (a+x)/2 recursion: weight 2^-(n-k+1), first window 2^-n
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = fmaf(wk, __builtin_amdgcn_sqrtf(fmaf(v[r].x, v[r].x, v[r].y * v[r].y)), acc[i][r]);
          } else if (p.cumu == CUMU_MAX) {   // np.max / np.min of K:141-143: a NaN window keeps the bin NaN
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = nan_max_nonneg(acc[i][r], fmaf(v[r].x, v[r].x, v[r].y * v[r].y));
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = nan_min(acc[i][r], fmaf(v[r].x, v[r].x, v[r].y * v[r].y));
          }
        }
      }
    }
    // ---- scale, fftshift (bin b -> (b + N/2) mod N), dB, waterfall cell (finish_frame's arithmetic) ----------------------
    int tid = threadIdx.x, n = plan.n;
    mr_opaque(tid, n);
    const int q4 = n / 4;
    const int g = p.hm_w > 0 ? n / p.hm_w : 0;   // bins per waterfall cell: any divisor of N
    float* const orow = p.out + (long long)frame * n;
    float* const red = reinterpret_cast<float*>(lds);   // [N] dB - adj in shifted order (waterfall only)
    if (g > 0) __syncthreads();   // the last pass's LDS reads are done
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int j = tid + i * T;
      if (j < q4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float lin = (CM == CUMU_PSD || p.cumu == CUMU_AVG) ? acc[i][r] : __builtin_amdgcn_sqrtf(acc[i][r]);
          lin *= p.scale;
          const float o = p.out_mode != OUT_LINEAR ? out_db(lin, p.out_mode, p.gain, p.min_amp) : lin;
          const int b = j + r * q4 + n / 2;
          const int sh = b < n ? b : b - n;
          orow[sh] = o;
          if (g > 0) red[sh] = p.adj ? o - p.adj[sh] : o;
        }
      }
    }
    if (g > 0) {
      __syncthreads();
      float* const hm_row = p.hm_rows ? p.hm_rows + (long long)frame * p.hm_w : nullptr;
      float* const hm_ring = (p.hm_ring && frame >= p.hm_first) ? p.hm_ring + ((p.hm_index0 + frame) % HM_ROWS) * p.hm_w : nullptr;
      // the cell maximum is np.max (K:195 through K:480): a NaN bin makes the cell NaN
      for (int cell = tid; cell < p.hm_w; cell += T) {
        const float* const c = red + cell * g;
        float hv = c[0];
        bool bad = hv != hv;
        for (int i = 1; i < g; ++i) {
          const float x = c[i];
          bad |= x != x;
          hv = fmaxf(hv, x);
        }
        if (bad) hv = __builtin_nanf("");
        if (hm_row) hm_row[cell] = hv;
        if (hm_ring) hm_ring[cell] = hv;
      }
      // (the next frame's first pass writes LDS behind a barrier)
    }
  }
