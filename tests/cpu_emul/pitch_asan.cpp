// TEST-ONLY, stand-alone: alsep_pitch_shift (csrc/pitch.h through reverb.hip, the unchanged kernel source on the CPU emulation) under
// AddressSanitizer.  Every buffer is a heap allocation of exactly the size the entry point is told, so a kernel index one element
// outside any of them aborts the run.  Geometries: both signs of the shift at the extremes of the ratio, an odd channel count, a signal
// shorter than a frame, one sample, and the largest frame (4097 bins: the fifth bin per thread of the recurrence); each with the
// smallest batch (4 frames: the most seams, the z segment at its tightest) and with a generous one, whose results must agree bit for
// bit.  Built and run by run_pitch_asan.sh; nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "alsep_common.h"

namespace {

struct Geometry { const char* name; int channels; int64_t n; int n_fft; double semitones; };

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double noise() {                                                             // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

int shift(alsep_ctx* ctx, const Geometry& g, const float* x, int frames_per_batch, std::vector<float>& out) {
    const double ratio = std::pow(2.0, g.semitones / 12.0);
    const int64_t need = alsep_pitch_shift_workspace_bytes(g.channels, g.n_fft, frames_per_batch, ratio);
    if (need < 0) { std::printf("%s: bad geometry\n", g.name); return 1; }
    char* ws = new char[(size_t)need];
    float* y = new float[(size_t)(g.channels * g.n)];
    const int rc = alsep_pitch_shift(ctx, x, g.channels, g.n, g.n, ratio, g.n_fft, frames_per_batch, y, g.n, ws, need);
    if (rc != ALSEP_OK) std::printf("%s: alsep_pitch_shift returned %d: %s\n", g.name, rc, ctx->err.c_str());
    out.assign(y, y + g.channels * g.n);
    delete[] y; delete[] ws;
    return rc != ALSEP_OK;
}

int run(alsep_ctx* ctx, const Geometry& g) {
    float* x = new float[(size_t)(g.channels * g.n)];
    for (int64_t i = 0; i < g.channels * g.n; ++i) x[i] = (float)(0.1 * noise() + 0.3 * std::sin(0.3456 * (double)(i % g.n)));
    std::vector<float> a, b;
    int bad = shift(ctx, g, x, 4, a) + shift(ctx, g, x, 64, b);
    delete[] x;
    if (bad) return 1;
    double peak = 0.0;
    for (float v : a) { if (!std::isfinite(v)) bad = 1; peak = std::fmax(peak, std::fabs((double)v)); }
    const bool same = std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
    std::printf("%s: peak %.3f, finite %s, batches of 4 and of 64 frames %s\n", g.name, peak, bad ? "NO" : "yes", same ? "agree bit for bit" : "DIFFER");
    return bad || !same || !(peak < 4.0);
}

}  // namespace

int main() {
    alsep_ctx ctx;
    const Geometry cases[] = {{"stereo +24", 2, 3001, 256, 24.0}, {"stereo -24", 2, 3001, 256, -24.0}, {"three channels +7", 3, 2500, 512, 7.0},
                              {"mono -5, n_fft 1024", 1, 4097, 1024, -5.0}, {"shorter than a frame", 2, 50, 256, 3.0}, {"one sample", 1, 1, 256, -13.0},
                              {"n_fft 8192", 1, 9001, 8192, 7.0}};
    int bad = 0;
    for (const Geometry& g : cases) bad += run(&ctx, g);
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
