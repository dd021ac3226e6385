// TEST-ONLY, stand-alone: the entry points of csrc/rmvpe.h (through nn.hip, the unchanged kernel source on the CPU emulation) under
// AddressSanitizer.  Every buffer is a heap allocation of exactly the size the entry point is told, so a kernel index one element outside
// any of them aborts the run.  Geometries: tracks of 1, 159, 160, 513 and 5280 samples (the shortest fold the reflection several times; an
// odd and an even frame count); a filterbank whose last band ends on the last bin; the frame padding at its limit (17 -> 32); the pool and
// the transposed convolution at one pixel, at odd sizes and into a channel slice that ends on the tensor's last channel; the GRU at every
// slicing of k (H = 16, 48, 256, 512) with one and two sequences; the decode with its peak on the first and the last bin.  Built and run by
// run_rmvpe_asan.sh; nothing here is loaded into Python.
#include <cmath>
#include <cstdio>

#include "alsep_common.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
float noise() {                                                              // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (float)((double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0);
}

float* filled(size_t n, float scale = 1.f) {
    float* p = new float[n];
    for (size_t i = 0; i < n; ++i) p[i] = scale * noise();
    return p;
}

int check(alsep_ctx* ctx, int rc, const char* what) {
    if (rc != ALSEP_OK) std::printf("%s returned %d: %s\n", what, rc, ctx->err.c_str());
    return rc != ALSEP_OK;
}

template <typename T>
int finite(const T* v, int64_t n, const char* what) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite((double)v[i])) { std::printf("%s[%lld] is not finite\n", what, (long long)i); return 1; }
    return 0;
}

int run_mel(alsep_ctx* ctx, int64_t n) {
    const int64_t T = alsep_rmvpe_frames(n);
    int bad = T != n / 160 + 1;
    float* audio = filled((size_t)n, 0.5f);
    float* win = new float[1024];
    for (int i = 0; i < 1024; ++i) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / 1024));
    float* tw = new float[2 * 512];
    for (int k = 0; k < 512; ++k) { tw[2 * k] = (float)std::cos(2.0 * M_PI * k / 1024); tw[2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / 1024); }
    float* basis = new float[128 * 513];
    for (int i = 0; i < 128 * 513; ++i) basis[i] = 0.25f;
    int32_t* bands = new int32_t[128 * 2];                                  // 5 bins each, 4 apart: band 127 ends on bin 512
    for (int b = 0; b < 128; ++b) { bands[2 * b] = 4 * b; bands[2 * b + 1] = 5; }
    float* lin = new float[(size_t)(T * 128)];
    float* logm = new float[(size_t)(T * 128)];
    bad += check(ctx, alsep_rmvpe_mel(ctx, audio, n, win, tw, basis, bands, lin, logm), "alsep_rmvpe_mel");
    bad += finite(lin, T * 128, "mel_lin") + finite(logm, T * 128, "mel_log");
    bad += check(ctx, alsep_rmvpe_mel(ctx, audio, n, win, tw, basis, bands, nullptr, logm), "alsep_rmvpe_mel (no linear output)");
    std::printf("mel: %lld samples, %lld frames%s\n", (long long)n, (long long)T, bad ? " FAILED" : "");
    delete[] audio; delete[] win; delete[] tw; delete[] basis; delete[] bands; delete[] lin; delete[] logm;
    return bad;
}

int run_pad(alsep_ctx* ctx, int64_t T, int64_t Tp, int C) {
    float* x = filled((size_t)(T * C));
    float* y = new float[(size_t)(Tp * C)];
    int bad = check(ctx, alsep_rmvpe_pad_frames(ctx, x, y, T, Tp, C, 0.5f, 1.f), "alsep_rmvpe_pad_frames");
    bad += finite(y, Tp * C, "padded");
    delete[] x; delete[] y;
    return bad;
}

int run_pool(alsep_ctx* ctx, int H, int W, int C, bool with_cat) {
    float* x = filled((size_t)H * W * C);
    float* y = new float[(size_t)(H / 2) * (W / 2) * C];
    float* cat = with_cat ? filled((size_t)H * W * 2 * C) : nullptr;       // the skip half ends on the last channel
    int bad = check(ctx, alsep_rmvpe_avgpool2(ctx, x, y, 1, H, W, C, cat, 2 * C, C), "alsep_rmvpe_avgpool2");
    bad += finite(y, (int64_t)(H / 2) * (W / 2) * C, "pooled");
    delete[] x; delete[] y; delete[] cat;
    return bad;
}

int run_tconv(alsep_ctx* ctx, int H, int W, int Cin, int Cout, int ct, int off) {
    float* x = filled((size_t)H * W * Cin);
    float* w = static_cast<float*>(std::aligned_alloc(16, sizeof(float) * 9 * Cin * Cout));
    for (int i = 0; i < 9 * Cin * Cout; ++i) w[i] = noise();
    float* scale = filled((size_t)Cout);
    float* shift = filled((size_t)Cout);
    float* y = filled((size_t)4 * H * W * ct);
    int bad = check(ctx, alsep_rmvpe_tconv3x3s2(ctx, x, w, scale, shift, y, 1, H, W, Cin, Cout, 1, ct, off), "alsep_rmvpe_tconv3x3s2");
    bad += finite(y, (int64_t)4 * H * W * ct, "tconv");
    delete[] x; std::free(w); delete[] scale; delete[] shift; delete[] y;
    return bad;
}

int run_gru(alsep_ctx* ctx, int T, int N, int H) {
    float* pre = filled((size_t)T * N * 6 * H);
    float* whh = filled((size_t)2 * H * 3 * H, 1.f / std::sqrt((float)H));
    float* bhh = filled((size_t)2 * 3 * H, 0.1f);
    float* h = new float[(size_t)T * N * 2 * H];
    int bad = check(ctx, alsep_nn_gru(ctx, pre, whh, bhh, h, T, N, H), "alsep_nn_gru");
    bad += finite(h, (int64_t)T * N * 2 * H, "h");
    for (int64_t i = 0; i < (int64_t)T * N * 2 * H && !bad; ++i)
        if (std::fabs(h[i]) > 1.f) { std::printf("|h[%lld]| > 1\n", (long long)i); bad = 1; }
    std::printf("gru: T %d, N %d, H %d%s\n", T, N, H, bad ? " FAILED" : "");
    delete[] pre; delete[] whh; delete[] bhh; delete[] h;
    return bad;
}

int run_decode(alsep_ctx* ctx, int64_t T) {
    float* sal = new float[(size_t)(T * 360)];
    for (int64_t i = 0; i < T * 360; ++i) sal[i] = 0.25f + 0.25f * noise();
    sal[0] = 0.9f;                                                          // frame 0: the peak on bin 0
    sal[(T - 1) * 360 + 359] = 0.95f;                                       // the last frame: the peak on bin 359
    double* f0 = new double[(size_t)T];
    int bad = check(ctx, alsep_rmvpe_sigmoid(ctx, sal, T * 360), "alsep_rmvpe_sigmoid");
    bad += check(ctx, alsep_rmvpe_decode(ctx, sal, T, 0.03f, f0), "alsep_rmvpe_decode");
    bad += finite(f0, T, "f0");
    delete[] sal; delete[] f0;
    return bad;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    int bad = 0;
    for (int64_t n : {(int64_t)1, (int64_t)159, (int64_t)160, (int64_t)513, (int64_t)5280}) bad += run_mel(&ctx, n);
    bad += run_pad(&ctx, 17, 32, 128) + run_pad(&ctx, 33, 64, 128) + run_pad(&ctx, 64, 64, 3);
    bad += run_pool(&ctx, 2, 2, 1, false) + run_pool(&ctx, 2, 4, 3, true) + run_pool(&ctx, 6, 128, 16, true);
    bad += run_tconv(&ctx, 1, 1, 1, 4, 4, 0) + run_tconv(&ctx, 1, 2, 8, 4, 8, 4) + run_tconv(&ctx, 3, 5, 16, 8, 16, 0) + run_tconv(&ctx, 3, 4, 16, 8, 11, 3);
    bad += run_gru(&ctx, 1, 1, 16) + run_gru(&ctx, 3, 2, 16) + run_gru(&ctx, 5, 1, 48) + run_gru(&ctx, 4, 2, 256) + run_gru(&ctx, 2, 1, 512);
    bad += run_decode(&ctx, 1) + run_decode(&ctx, 5) + run_decode(&ctx, 9);
    // refusals come before any launch
    float a = 0.f, b = 0.f;
    double d = 0.0;
    bad += alsep_rmvpe_frames(0) != -1 || alsep_rmvpe_frames((int64_t)160 << 20) != -1;
    bad += alsep_rmvpe_pad_frames(&ctx, &a, &b, 16, 32, 1, 1.f, 0.f) == ALSEP_OK;              // 16 frames cannot give 16 reflected ones
    bad += alsep_rmvpe_avgpool2(&ctx, &a, &b, 1, 3, 2, 1, nullptr, 0, 0) == ALSEP_OK;          // an odd height
    bad += alsep_rmvpe_tconv3x3s2(&ctx, &a, &a, &a, &a, &b, 1, 1, 1, 1, 6, 1, 6, 0) == ALSEP_OK;   // channels not in fours
    bad += alsep_rmvpe_tconv3x3s2(&ctx, &a, &a, &a, &a, &b, 1, 1, 1, 1, 4, 1, 6, 4) == ALSEP_OK;   // the slice ends beyond the tensor
    bad += alsep_nn_gru(&ctx, &a, &a, &a, &b, 1, 1, 24) == ALSEP_OK;                            // H % 16
    bad += alsep_rmvpe_decode(&ctx, &a, 0, 0.03f, &d) == ALSEP_OK;
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
