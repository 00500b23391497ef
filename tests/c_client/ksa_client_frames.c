/* A plain C99 client of the batched host-memory zeroSpan entry point: 256 capture blocks in page-locked memory from
 * ksa_host_alloc go through ONE ksa_frames_c64 call.  Built and run by tests/test_gpu_host_frames.py on the GPU box:
 *   gcc -std=c99 -O2 -I include tests/c_client/ksa_client_frames.c -L prgs-sdr-kspecanal_amd -lksa -lm ...
 * The input is an on-bin tone A*exp(j*2*pi*k*n/N) under a rectangular window (reads 2A at bin k, K:391): bin k is the
 * peak of Fft.Max, at 10*log10(2A) - gain dB, and 256 frames leave the waterfall ring at row 256 % 128 = 0. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "ksa.h"

#define CHECK(call)                                                             \
  do {                                                                          \
    if ((call) != 0) {                                                          \
      fprintf(stderr, "%s failed: %s\n", #call, ksa_last_error());              \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

int main(void) {
  enum { N = 1024, FULL = 8192, XRES = 64, FRAMES = 256 };
  const double q = 0.5, amp = 0.25, gain = 19.1;
  const int kbin = 100;
  const double pi = 3.14159265358979323846;
  static float win[N], cur[N], mx[N], mn[N], av[N];
  static int32_t starts[64];
  int nwin = 0, i, f, peak = 0;
  void* mem = NULL;
  float* iq;
  ksa_config cfg;
  ksa_engine* e = NULL;
  int32_t hm_index = -1;
  int64_t seen = -1;
  double want;
  for (i = 0; i < (int)(FULL / (N * q)); ++i) {   /* window starts exactly as K:368 / K:386-390 */
    const int s = (int)(i * N * q);
    if (s + N > FULL) break;
    starts[nwin++] = s;
  }
  for (i = 0; i < N; ++i) win[i] = 1.0f;
  CHECK(ksa_host_alloc(&mem, (int64_t)FRAMES * FULL * 2 * (int64_t)sizeof(float)));
  iq = (float*)mem;
  for (f = 0; f < FRAMES; ++f)
    for (i = 0; i < FULL; ++i) {
      const double ph = 2 * pi * kbin * (double)i / N;
      iq[(size_t)2 * ((size_t)f * FULL + i)] = (float)(amp * cos(ph));
      iq[(size_t)2 * ((size_t)f * FULL + i) + 1] = (float)(amp * sin(ph));
    }
  memset(&cfg, 0, sizeof cfg);
  cfg.abi_version = KSA_ABI_VERSION;
  cfg.device = 0;
  cfg.fft_size = N;
  cfg.full_size = FULL;
  cfg.num_windows = nwin;
  cfg.window_starts = starts;
  cfg.window = win;
  cfg.mag_scale = 2.0 * 1.0 / N;   /* winAdj = 1 for the rectangular window, K:373 + K:391 */
  cfg.cumu_mode = KSA_CUMU_AVG;
  cfg.gain = (float)gain;
  cfg.min_amp = (float)((1.0 / 256) * 0.00001);
  cfg.hm_width = XRES;
  cfg.max_frames = FRAMES;
  cfg.u8_offset = 127.5f;
  cfg.u8_scale = 127.5f;
  CHECK(ksa_create(&cfg, &e));
  CHECK(ksa_frames_c64(e, iq, FRAMES, 0, FRAMES, NULL, NULL, 1));
  CHECK(ksa_read_state(e, cur, mx, mn, av, NULL, &hm_index, &seen));
  for (i = 1; i < N; ++i)
    if (mx[i] > mx[peak]) peak = i;
  want = 10.0 * log10(2.0 * amp) - gain;
  /* fftshifted spectrum: bin k sits at index k + N/2 */
  if (peak != kbin + N / 2 || fabs(mx[peak] - want) > 1e-3) {
    fprintf(stderr, "Max peak at %d (%.4f dB), want %d (%.4f dB)\n", peak, mx[peak], kbin + N / 2, want);
    return 1;
  }
  if (hm_index != 0 || seen != FRAMES) {
    fprintf(stderr, "hm_index %d frames %lld, want 0 and %d\n", (int)hm_index, (long long)seen, FRAMES);
    return 1;
  }
  ksa_destroy(e);
  CHECK(ksa_host_free(mem));
  printf("c frames client ok: peak %d %.4f dB, hm_index %d\n", peak, mx[peak], (int)hm_index);
  return 0;
}
