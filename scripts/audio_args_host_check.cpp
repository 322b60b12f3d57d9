// Stand-alone host check of the audio entry points' argument handling (include/dv3hip.h, the `_n` siblings of ABI 49
// and dv3_gl_project_momentum_f32):
// every call below must be refused with DV3_EINVAL on the host -- an unsupported n_fft, too few frames for the framing,
// a hop above n_fft, a missing pointer, a momentum outside [0, 1) -- so nothing is launched and no GPU is needed.  Meant for a sanitizer build of
// the host side of csrc/audio.hip (the frame / sample / offset arithmetic in front of the launches):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       deepvoice3_pytorch_amd/csrc/audio.hip scripts/audio_args_host_check.cpp -o build_tmp/audio_args_host_check
//   ./build_tmp/audio_args_host_check
//
// It links audio.hip alone, so it brings its own dv3_set_error (api.hip's sits among the other kernels' switches).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/dv3hip.h"

static char g_err[512];
void dv3_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int g_failed = 0;
static void expect_einval(const char* what, int rc, const char* needle) {
  const bool ok = rc == DV3_EINVAL && (!needle || strstr(g_err, needle));
  if (!ok) {
    ++g_failed;
    printf("FAIL %s: rc %d, message \"%s\"\n", what, rc, g_err);
  }
  g_err[0] = 0;
}

int main() {
  // never dereferenced on these paths: the host only tests them against NULL
  float buf[8] = {0};
  int32_t ibuf[8] = {0};
  int64_t lbuf[8] = {0};
  float *p = buf, *o = buf + 4;
  alignas(8) float cbuf[8] = {0};
  float* c = cbuf;
  const int32_t B = 2;
  const int32_t bad[] = {4096, 768, 256, 0, -1024, 1023, INT32_MAX, INT32_MIN};
  for (int32_t nf : bad) {
    const char* m = "n_fft";
    expect_einval("istft_frames n_fft", dv3_istft_frames_f32_n(p, p, o, B, 12, nf, nullptr), m);
    expect_einval("overlap_add n_fft", dv3_overlap_add_f32_n(p, o, B, 12, 128, nf, nullptr), m);
    expect_einval("gl_project n_fft", dv3_gl_project_f32_n(p, p, o, B, 12, 128, nf, nullptr), m);
    expect_einval("stft_phase n_fft", dv3_stft_phase_f32_n(p, o, nullptr, nullptr, B, 12, 128, nf, nullptr), m);
    expect_einval("lws_stft n_fft", dv3_lws_stft_f32_n(p, p, o, nullptr, nullptr, B, 12, 128, 1000, nf, nullptr), m);
    expect_einval("lws_istft_frames n_fft", dv3_lws_istft_frames_f32_n(p, p, p, o, B, 12, nf, nullptr), m);
    expect_einval("lws_overlap_add n_fft", dv3_lws_overlap_add_f32_n(p, o, B, 12, 128, nf, nullptr), m);
    expect_einval("lws_gl_project n_fft", dv3_lws_gl_project_f32_n(p, p, p, p, o, B, 12, 128, nf, nullptr), m);
    expect_einval("gl_istft_items n_fft", dv3_gl_istft_items_f32_n(p, p, p, o, B, 12, 128, ibuf, 1, nf, nullptr), m);
    expect_einval("overlap_add_items n_fft", dv3_overlap_add_items_f32_n(p, o, B, 12, 128, ibuf, 1, nf, nullptr), m);
    expect_einval("gl_project_items n_fft", dv3_gl_project_items_f32_n(p, p, p, p, o, B, 12, 128, ibuf, 1, nf, nullptr), m);
    expect_einval("analysis_items n_fft", dv3_analysis_items_f32_n(p, lbuf, ibuf, B, 12, 128, 0.97f, p, nullptr, p, nullptr, 80,
                                                                   -100.f, 20.f, o, nullptr, nf, nullptr), m);
    for (int32_t lws = 0; lws < 2; ++lws) {
      expect_einval("gl_project_momentum n_fft", dv3_gl_project_momentum_f32(p, p, p, p, c, o, B, 12, 128, nullptr, lws, nf, 0.99f, 1, nullptr), m);
      expect_einval("gl_project_momentum items n_fft", dv3_gl_project_momentum_f32(p, p, p, p, c, o, B, 12, 128, ibuf, lws, nf, 0.99f, 0, nullptr), m);
    }
  }
  const int32_t sizes[] = {512, 1024, 2048};
  for (int32_t nf : sizes) {
    const int32_t hop = nf / 4, hop2 = 3 * nf / 16;
    // too few frames: (T + 1) * hop - n_fft <= 0 on the lws framing, hop * (T - 1) <= n_fft / 2 on the torch one
    expect_einval("lws_overlap_add T=3", dv3_lws_overlap_add_f32_n(p, o, B, 3, hop, nf, nullptr), nullptr);
    expect_einval("lws_overlap_add T=4 at 3n/16", dv3_lws_overlap_add_f32_n(p, o, B, 4, hop2, nf, nullptr), nullptr);
    expect_einval("lws_gl_project T=3", dv3_lws_gl_project_f32_n(p, p, p, p, o, B, 3, hop, nf, nullptr), nullptr);
    expect_einval("lws_stft L=0", dv3_lws_stft_f32_n(p, p, o, nullptr, nullptr, B, 3, hop, 0, nf, nullptr), nullptr);
    expect_einval("lws_stft frames do not frame L", dv3_lws_stft_f32_n(p, p, o, nullptr, nullptr, B, 12, hop, 2 * hop, nf, nullptr),
                  "do not frame");
    expect_einval("lws_stft L past the frames", dv3_lws_stft_f32_n(p, p, o, nullptr, nullptr, B, 12, hop, 13 * hop - nf + 1, nf,
                                                                   nullptr), "do not frame");
    expect_einval("stft_phase T=3", dv3_stft_phase_f32_n(p, o, nullptr, nullptr, B, 3, hop, nf, nullptr), "reflect");
    expect_einval("gl_project T=3", dv3_gl_project_f32_n(p, p, o, B, 3, hop, nf, nullptr), "reflect");
    expect_einval("gl_istft_items T=3", dv3_gl_istft_items_f32_n(p, p, p, o, B, 3, hop, ibuf, 1, nf, nullptr), nullptr);
    expect_einval("gl_istft_items torch T=3", dv3_gl_istft_items_f32_n(p, p, nullptr, o, B, 3, hop, ibuf, 0, nf, nullptr), nullptr);
    expect_einval("overlap_add_items T=3", dv3_overlap_add_items_f32_n(p, o, B, 3, hop, ibuf, 1, nf, nullptr), nullptr);
    expect_einval("gl_project_items T=4 at 3n/16", dv3_gl_project_items_f32_n(p, p, p, p, o, B, 4, hop2, ibuf, 1, nf, nullptr), nullptr);
    // a hop above the frame, extreme counts, missing pointers
    expect_einval("overlap_add hop > n_fft", dv3_overlap_add_f32_n(p, o, B, 12, nf + 1, nf, nullptr), nullptr);
    expect_einval("lws_overlap_add hop > n_fft", dv3_lws_overlap_add_f32_n(p, o, B, 12, nf + 1, nf, nullptr), nullptr);
    expect_einval("analysis_items hop > n_fft", dv3_analysis_items_f32_n(p, lbuf, ibuf, B, 12, nf + 1, 0.97f, p, nullptr, p, nullptr,
                                                                         80, -100.f, 20.f, o, nullptr, nf, nullptr), nullptr);
    expect_einval("analysis_items no output", dv3_analysis_items_f32_n(p, lbuf, ibuf, B, 12, hop, 0.97f, p, nullptr, p, nullptr, 80,
                                                                       -100.f, 20.f, nullptr, nullptr, nf, nullptr), nullptr);
    expect_einval("analysis_items mel without basis", dv3_analysis_items_f32_n(p, lbuf, ibuf, B, 12, hop, 0.97f, p, nullptr, nullptr,
                                                                               nullptr, 80, -100.f, 20.f, nullptr, o, nf, nullptr), nullptr);
    expect_einval("istft_frames B=0", dv3_istft_frames_f32_n(p, p, o, 0, 12, nf, nullptr), nullptr);
    expect_einval("istft_frames no mag", dv3_istft_frames_f32_n(nullptr, p, o, B, 12, nf, nullptr), nullptr);
    expect_einval("lws_istft_frames no window", dv3_lws_istft_frames_f32_n(p, p, nullptr, o, B, 12, nf, nullptr), nullptr);
    expect_einval("overlap_add T=1", dv3_overlap_add_f32_n(p, o, B, 1, hop, nf, nullptr), nullptr);
    expect_einval("overlap_add hop=0", dv3_overlap_add_f32_n(p, o, B, 12, 0, nf, nullptr), nullptr);
    // counts whose sample total does not fit an int: refused before the total is formed
    expect_einval("lws_overlap_add huge T", dv3_lws_overlap_add_f32_n(p, o, B, INT32_MAX, hop, nf, nullptr), nullptr);
    expect_einval("lws_overlap_add 2^31 samples", dv3_lws_overlap_add_f32_n(p, o, B, (1 << 30) / hop * 2, hop, nf, nullptr), nullptr);
    expect_einval("overlap_add huge T", dv3_overlap_add_f32_n(p, o, B, INT32_MAX, hop, nf, nullptr), nullptr);
    expect_einval("stft_phase huge T", dv3_stft_phase_f32_n(p, o, nullptr, nullptr, B, INT32_MAX - 1, hop, nf, nullptr), nullptr);
    expect_einval("gl_project huge T", dv3_gl_project_f32_n(p, p, o, B, 1 << 30, hop, nf, nullptr), nullptr);
    expect_einval("lws_stft huge T", dv3_lws_stft_f32_n(p, p, o, nullptr, nullptr, B, INT32_MAX, hop, 1000, nf, nullptr), nullptr);
    expect_einval("lws_gl_project huge T", dv3_lws_gl_project_f32_n(p, p, p, p, o, B, INT32_MAX, hop, nf, nullptr), nullptr);
    expect_einval("gl_istft_items huge T", dv3_gl_istft_items_f32_n(p, p, p, o, B, INT32_MAX, hop, ibuf, 1, nf, nullptr), nullptr);
    expect_einval("overlap_add_items huge T", dv3_overlap_add_items_f32_n(p, o, B, INT32_MAX, hop, ibuf, 0, nf, nullptr), nullptr);
    expect_einval("gl_project_items huge T", dv3_gl_project_items_f32_n(p, p, p, p, o, B, 1 << 30, hop, ibuf, 1, nf, nullptr), nullptr);
    expect_einval("gl_project_items no tlen", dv3_gl_project_items_f32_n(p, p, p, p, o, B, 12, hop, nullptr, 1, nf, nullptr), nullptr);
    // the momentum projection: both framings, the whole batch (tlen NULL) and per item, first call and later ones
    for (int32_t form = 0; form < 8; ++form) {
      const int32_t lws = form & 1, first = (form >> 2) & 1;
      const int32_t* tl = (form & 2) ? ibuf : nullptr;
      const float* aw = lws ? p : nullptr;                       // the torch framing takes no window tables
      expect_einval("gl_project_momentum no cprev", dv3_gl_project_momentum_f32(p, p, aw, aw, nullptr, o, B, 12, hop, tl, lws, nf, 0.99f, first, nullptr), "cprev");
      expect_einval("gl_project_momentum odd cprev", dv3_gl_project_momentum_f32(p, p, aw, aw, c + 1, o, B, 12, hop, tl, lws, nf, 0.99f, first, nullptr), "cprev");
      expect_einval("gl_project_momentum alpha 1", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 12, hop, tl, lws, nf, 1.0f, first, nullptr), "alpha");
      expect_einval("gl_project_momentum alpha -0.1", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 12, hop, tl, lws, nf, -0.1f, first, nullptr), "alpha");
      expect_einval("gl_project_momentum alpha nan", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 12, hop, tl, lws, nf, NAN, first, nullptr), "alpha");
      expect_einval("gl_project_momentum alpha inf", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 12, hop, tl, lws, nf, INFINITY, first, nullptr), "alpha");
      expect_einval("gl_project_momentum T=3", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 3, hop, tl, lws, nf, 0.99f, first, nullptr), "fewer");
      expect_einval("gl_project_momentum T=1", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 1, hop, tl, lws, nf, 0.99f, first, nullptr), nullptr);
      expect_einval("gl_project_momentum hop > n_fft", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 12, nf + 1, tl, lws, nf, 0.99f, first, nullptr), nullptr);
      expect_einval("gl_project_momentum hop=0", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 12, 0, tl, lws, nf, 0.99f, first, nullptr), nullptr);
      expect_einval("gl_project_momentum B=0", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, 0, 12, hop, tl, lws, nf, 0.99f, first, nullptr), nullptr);
      expect_einval("gl_project_momentum huge T", dv3_gl_project_momentum_f32(p, p, aw, aw, c, o, B, 1 << 30, hop, tl, lws, nf, 0.99f, first, nullptr), nullptr);
      expect_einval("gl_project_momentum no frames", dv3_gl_project_momentum_f32(p, p, aw, aw, c, nullptr, B, 12, hop, tl, lws, nf, 0.99f, first, nullptr), nullptr);
      expect_einval("gl_project_momentum no mag", dv3_gl_project_momentum_f32(p, nullptr, aw, aw, c, o, B, 12, hop, tl, lws, nf, 0.99f, first, nullptr), nullptr);
    }
    expect_einval("gl_project_momentum T=4 at 3n/16", dv3_gl_project_momentum_f32(p, p, p, p, c, o, B, 4, hop2, ibuf, 1, nf, 0.5f, 0, nullptr), "fewer");
    expect_einval("gl_project_momentum lws without windows", dv3_gl_project_momentum_f32(p, p, nullptr, nullptr, c, o, B, 12, hop, nullptr, 1, nf, 0.5f, 0, nullptr), nullptr);
  }
  // the entry points without n_fft are the 1024 instantiation: the same refusals
  expect_einval("lws_overlap_add (1024) T=3", dv3_lws_overlap_add_f32(p, o, B, 3, 256, nullptr), nullptr);
  expect_einval("stft_phase (1024) T=3", dv3_stft_phase_f32(p, o, nullptr, nullptr, B, 3, 256, nullptr), "reflect");
  expect_einval("overlap_add (1024) hop 1025", dv3_overlap_add_f32(p, o, B, 12, 1025, nullptr), nullptr);
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("audio argument checks ok\n");
  return 0;
}
