// TEST-ONLY, stand-alone: alsep_reverb_apply (csrc/reverb.hip, the unchanged kernel source on the CPU emulation) under AddressSanitizer.
// Every buffer is a heap allocation of exactly the size the entry point is told, so a kernel index one element outside any of them
// aborts the run.  Three geometries of tests/reverb_apply_cases.py -- tiny_stereo (9 blocks, ragged last one), three_ch (odd channel
// count, odd L, a pre-delay) and unit_ir (L = 1) -- each with a one-block workspace and with a generous one, checked against a direct
// double convolution.  Built and run by run_reverb_apply_asan.sh; nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "alsep_common.h"

namespace {

struct Geometry { const char* name; int channels; int64_t n, taps, pre; int log2_block; };

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double noise() {                                                             // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

int run(alsep_ctx* ctx, const Geometry& g, int blocks_per_batch) {
    float* dry = new float[(size_t)(g.channels * g.n)];
    float* out = new float[(size_t)(g.channels * g.n)];
    double* ir = new double[(size_t)g.taps];
    for (int64_t i = 0; i < g.channels * g.n; ++i) dry[i] = (float)(0.25 * noise());
    double energy = 0.0;
    for (int64_t j = 0; j < g.taps; ++j) { ir[j] = j ? noise() * std::exp(-6.9 * (double)j / (double)g.taps) : 1.0; energy += ir[j] * ir[j]; }
    for (int64_t j = 0; j < g.taps; ++j) ir[j] /= std::sqrt(energy);
    const int64_t need = alsep_reverb_apply_workspace_bytes(g.taps, g.log2_block, blocks_per_batch);
    if (need < 0) { std::printf("%s: bad geometry\n", g.name); return 1; }
    char* ws = new char[(size_t)need];
    const int rc = alsep_reverb_apply(ctx, dry, g.channels, g.n, g.n, ir, g.taps, g.pre, 0.7, g.log2_block, out, g.n, ws, need);
    if (rc != ALSEP_OK) { std::printf("%s: alsep_reverb_apply returned %d: %s\n", g.name, rc, ctx->err.c_str()); return 1; }
    double worst = 0.0;
    for (int c = 0; c < g.channels; ++c)
        for (int64_t o = 0; o < g.n; ++o) {
            double wet = 0.0;
            for (int64_t j = 0, t = o - g.pre; j < g.taps && j <= t; ++j) wet += ir[j] * (double)dry[c * g.n + t - j];
            double v = (double)dry[c * g.n + o] + 0.7 * wet;
            v = v < -1.0 ? -1.0 : v > 1.0 ? 1.0 : v;
            worst = std::fmax(worst, std::fabs((double)out[c * g.n + o] - v));
        }
    std::printf("%s, %d block(s) per batch: max|out - direct| = %.3e\n", g.name, blocks_per_batch, worst);
    delete[] ws; delete[] ir; delete[] out; delete[] dry;
    return worst <= 5.9604644775390625e-8 ? 0 : 1;                           // 2^-24
}

}  // namespace

int main() {
    alsep_ctx ctx;
    const Geometry cases[] = {{"tiny_stereo", 2, 6001, 300, 0, 0}, {"three_ch", 3, 5000, 257, 8, 0}, {"unit_ir", 2, 3000, 1, 0, 0},
                              {"unit_ir, 2-point blocks", 2, 3000, 1, 0, 1}, {"delay_past_end", 2, 4000, 300, 6000, 0}};
    int bad = 0;
    for (const Geometry& g : cases) bad += run(&ctx, g, 1) + run(&ctx, g, 64);
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
