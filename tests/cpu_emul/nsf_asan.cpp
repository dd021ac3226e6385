// TEST-ONLY, stand-alone: the entry points of csrc/nsf.h (through nn.hip, the unchanged kernel source on the CPU emulation) under
// AddressSanitizer.  Every buffer is a heap allocation of exactly the size the entry point is told (16-byte aligned where the kernels use
// 16-byte accesses), so a kernel index one element outside any of them aborts the run.  Geometries: the source at 1, 2, 65 and 1025 frames
// (the last crosses the scan's chunk of 1024) at 6 and 400 samples a frame; the convolution at one position, below its halo, across a tile
// edge, with every optional operand and with 8 channels (the masked tile); conv_post at one position and across a tile; the transposed
// convolution at every (kernel, stride) of the kernel tests -- (16, 4) of the v1 32k configuration and (16, 2), eight taps a phase, among
// them -- and the largest source stride.  Built and run by run_nsf_asan.sh;
// nothing here is loaded into Python.
#include <cmath>
#include <cstdio>

#include "alsep_common.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
float noise() {                                                              // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (float)((double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0);
}

float* filled(size_t n, float scale = 1.f) {                                 // exactly n floats; the tensors with channels are whole 16 bytes
    float* p = static_cast<float*>(n % 4 ? std::malloc(sizeof(float) * n) : std::aligned_alloc(16, sizeof(float) * n));
    for (size_t i = 0; i < n; ++i) p[i] = scale * noise();
    return p;
}

int check(alsep_ctx* ctx, int rc, const char* what) {
    if (rc != ALSEP_OK) std::printf("%s returned %d: %s\n", what, rc, ctx->err.c_str());
    return rc != ALSEP_OK;
}

int bounded(const float* v, int64_t n, float lim, const char* what) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || std::fabs(v[i]) > lim) { std::printf("%s[%lld] = %g\n", what, (long long)i, (double)v[i]); return 1; }
    return 0;
}

int run_source(alsep_ctx* ctx, int64_t T, int upp) {
    float* f0 = filled((size_t)T);
    for (int64_t t = 0; t < T; ++t) f0[t] = (t % 5 == 3) ? 0.f : 600.f + 500.f * f0[t];
    float* nz = filled((size_t)(T * upp));
    float* har = filled((size_t)(T * upp));
    const int64_t bytes = alsep_nsf_source_workspace_bytes(T);
    void* ws = std::malloc((size_t)bytes);
    int bad = check(ctx, alsep_nsf_source(ctx, f0, T, upp, 40000, nz, 1.f, 0.f, har, ws, bytes), "alsep_nsf_source");
    bad += bounded(har, T * upp, 1.f, "har");
    std::printf("source: %lld frames of %d%s\n", (long long)T, upp, bad ? " FAILED" : "");
    std::free(f0); std::free(nz); std::free(har); std::free(ws);
    return bad;
}

int run_conv(alsep_ctx* ctx, int64_t L, int Cin, int Cout, int K, int d, bool extras) {
    float* x = filled((size_t)L * Cin);
    float* w = filled((size_t)K * Cin * Cout, 1.f / std::sqrt((float)(Cin * K)));
    float* bias = extras ? filled((size_t)Cout) : nullptr;
    float* res = extras ? filled((size_t)L * Cout) : nullptr;
    float* acc = extras ? filled((size_t)L * Cout) : nullptr;
    float* y = filled((size_t)L * Cout);
    int bad = check(ctx, alsep_nsf_conv1d(ctx, x, w, bias, res, acc, y, L, Cin, Cout, K, d, 0.1f, extras ? 1 : 0, extras ? 1.f / 3.f : 1.f),
                    "alsep_nsf_conv1d");
    bad += bounded(y, L * Cout, 100.f, "conv");
    std::printf("conv1d: L %lld, %d -> %d, K %d, d %d%s\n", (long long)L, Cin, Cout, K, d, bad ? " FAILED" : "");
    std::free(x); std::free(w); std::free(bias); std::free(res); std::free(acc); std::free(y);
    return bad;
}

int run_post(alsep_ctx* ctx, int64_t L, int C) {
    float* x = filled((size_t)L * C);
    float* w = filled((size_t)7 * C, 0.2f);
    float* y = filled((size_t)L);
    int bad = check(ctx, alsep_nsf_conv_post(ctx, x, w, y, L, C), "alsep_nsf_conv_post");
    bad += bounded(y, L, 1.f, "post");
    std::free(x); std::free(w); std::free(y);
    return bad;
}

int run_tconv(alsep_ctx* ctx, int64_t L, int Cin, int Cout, int K, int u, int s) {
    const int ks = s > 1 ? 2 * s : 1;
    float* x = filled((size_t)L * Cin);
    float* w = filled((size_t)K * Cin * Cout, 1.f / std::sqrt((float)(Cin * K)));
    float* bias = filled((size_t)Cout);
    float* har = filled((size_t)(L * u * s));
    float* nw = filled((size_t)ks * Cout, 1.f / std::sqrt((float)ks));
    float* nb = filled((size_t)Cout);
    float* y = filled((size_t)(L * u) * Cout);
    int bad = check(ctx, alsep_nsf_tconv1d(ctx, x, w, bias, har, nw, nb, y, L, Cin, Cout, K, u, s), "alsep_nsf_tconv1d");
    bad += bounded(y, L * u * Cout, 100.f, "tconv");
    std::printf("tconv1d: L %lld, %d -> %d, K %d, u %d, s %d%s\n", (long long)L, Cin, Cout, K, u, s, bad ? " FAILED" : "");
    std::free(x); std::free(w); std::free(bias); std::free(har); std::free(nw); std::free(nb); std::free(y);
    return bad;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    int bad = 0;
    for (int64_t T : {(int64_t)1, (int64_t)2, (int64_t)65, (int64_t)1025}) bad += run_source(&ctx, T, 6) + run_source(&ctx, T, 400);
    bad += run_conv(&ctx, 1, 16, 16, 3, 1, false) + run_conv(&ctx, 1, 16, 16, 3, 1, true) + run_conv(&ctx, 17, 16, 32, 7, 3, true);
    bad += run_conv(&ctx, 130, 32, 16, 11, 5, true) + run_conv(&ctx, 9, 192, 32, 7, 1, false) + run_conv(&ctx, 257, 64, 64, 3, 5, true);
    bad += run_conv(&ctx, 21, 8, 24, 5, 2, true) + run_conv(&ctx, 5, 24, 8, 3, 1, false);
    bad += run_post(&ctx, 1, 16) + run_post(&ctx, 130, 32) + run_post(&ctx, 67, 8);
    bad += run_tconv(&ctx, 1, 32, 16, 4, 2, 1) + run_tconv(&ctx, 5, 32, 16, 7, 3, 2) + run_tconv(&ctx, 13, 64, 32, 16, 10, 40);
    bad += run_tconv(&ctx, 7, 32, 16, 24, 12, 200) + run_tconv(&ctx, 140, 16, 8, 16, 6, 2) + run_tconv(&ctx, 5, 32, 16, 16, 4, 8);
    bad += run_tconv(&ctx, 3, 16, 16, 16, 2, 1);                            // 8 taps a phase, the most
    // refusals come before any launch
    alignas(16) float a[4] = {0.f, 0.f, 0.f, 0.f};
    alignas(16) float b[4] = {0.f, 0.f, 0.f, 0.f};
    alignas(16) double ws[8];
    bad += alsep_nsf_source_workspace_bytes(0) != -1;
    bad += alsep_nsf_source(&ctx, a, 0, 6, 40000, a, 1.f, 0.f, b, ws, sizeof(ws)) == ALSEP_OK;                // no frames
    bad += alsep_nsf_source(&ctx, a, 1, 1025, 40000, a, 1.f, 0.f, b, ws, sizeof(ws)) == ALSEP_OK;             // upp above 1024
    bad += alsep_nsf_source(&ctx, a, 1, 1, 40000, a, 1.f, 0.f, b, ws, 8) == ALSEP_OK;                         // a workspace too small
    bad += alsep_nsf_conv1d(&ctx, a, a, nullptr, nullptr, nullptr, b, 1, 12, 16, 3, 1, 1.f, 0, 1.f) == ALSEP_OK;   // channels not in eights
    bad += alsep_nsf_conv1d(&ctx, a, a, nullptr, nullptr, nullptr, b, 1, 16, 16, 4, 1, 1.f, 0, 1.f) == ALSEP_OK;   // an even kernel
    bad += alsep_nsf_conv1d(&ctx, a, a, nullptr, nullptr, nullptr, b, 1, 16, 16, 3, 6, 1.f, 0, 1.f) == ALSEP_OK;   // dilation above 5
    bad += alsep_nsf_conv1d(&ctx, a, a, nullptr, nullptr, nullptr, a, 1, 16, 16, 3, 1, 1.f, 0, 1.f) == ALSEP_OK;   // the output over the input
    bad += alsep_nsf_conv_post(&ctx, a, a, b, 1, 12) == ALSEP_OK;
    bad += alsep_nsf_tconv1d(&ctx, a, a, a, a, a, a, b, 1, 16, 16, 5, 2, 1) == ALSEP_OK;                      // K - u odd
    bad += alsep_nsf_tconv1d(&ctx, a, a, a, a, a, a, b, 1, 16, 16, 2, 4, 1) == ALSEP_OK;                      // K < u
    bad += alsep_nsf_tconv1d(&ctx, a, a, a, a, a, a, b, 1, 16, 16, 18, 2, 1) == ALSEP_OK;                     // K > 8 u
    bad += alsep_nsf_tconv1d(&ctx, a, a, a, a, a, a, b, 1, 16, 16, 4, 2, 3) == ALSEP_OK;                      // an odd source stride
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
