// TEST-ONLY, stand-alone: the mastering entry points (csrc/master.h through reverb.hip, the unchanged kernel source on the CPU emulation)
// under AddressSanitizer.  Every buffer is a heap allocation of exactly the size the entry point is told, so a kernel index one element
// outside any of them aborts the run.  Shapes: the small ones of tests/test_remaster.py -- 10007 samples in 4 pieces of 2501 (a tail of 3),
// one piece of 2999, one frame of 256, n_fft 4096 at 3 * 4096 + 5; convolutions shorter than, equal to and no multiple of a block's
// payload; sliding maxima at n = 2 w - 1 and at w = 4095; the scan at 200 samples in chunks of 64, at 7 samples and at the default chunk.
// Built and run by run_master_asan.sh; nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "alsep_common.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double noise() {                                                             // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

double* track(int64_t n, double gain) {
    double* x = new double[(size_t)n];
    for (int64_t i = 0; i < n; ++i) x[i] = gain * (0.1 * noise() + 0.3 * std::sin(0.0627 * (double)i));
    return x;
}

int g_bad = 0;
void expect(alsep_ctx* ctx, const char* what, int rc, int want = ALSEP_OK) {
    if (rc != want) { std::printf("%s returned %d (expected %d): %s\n", what, rc, want, ctx->err.c_str()); ++g_bad; }
}
void finite(const char* what, const double* x, int64_t n) {
    for (int64_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) { std::printf("%s: element %lld is not finite\n", what, (long long)i); ++g_bad; return; }
}

double* twiddles(int n_fft) {
    const double pi = 3.14159265358979323846;
    double* tw = new double[2 * (size_t)n_fft];
    for (int m = 0; m < n_fft; ++m) { tw[2 * m] = std::cos(2.0 * pi * m / n_fft); tw[2 * m + 1] = -std::sin(2.0 * pi * m / n_fft); }
    return tw;
}

// levels, spectrum and "same" convolution of one stereo track of n samples in d pieces of p
void analysis(alsep_ctx* ctx, int64_t n, int d, int64_t p, int n_fft, int log2_block, int blocks_per_batch) {
    const int64_t wsb = alsep_master_workspace_bytes();
    char* ws = new char[(size_t)wsb];
    double* lr = track(2 * n, 1.0);
    double* ms = new double[2 * (size_t)n];
    expect(ctx, "alsep_master_midside", alsep_master_midside(ctx, lr, n, n, 0.7, ms, n));
    double* peak = new double[1];
    expect(ctx, "alsep_master_peak", alsep_master_peak(ctx, lr, 2, n, n, peak, ws, wsb));
    double* sums = new double[(size_t)d];
    expect(ctx, "alsep_master_piece_sumsq", alsep_master_piece_sumsq(ctx, ms, n, d, p, 1.0, 0, sums, ws, wsb));
    expect(ctx, "alsep_master_piece_sumsq (clip)", alsep_master_piece_sumsq(ctx, ms, n, d, p, 3.0, 1, sums, ws, wsb));
    finite("piece sums", sums, d);
    std::vector<int32_t> pieces;
    for (int j = 0; j < d; j += 2) pieces.push_back(j);
    if (d > 1) pieces.back() = d - 1;                                       // the last piece: its frames end nearest to the end of the track
    double* tw = twiddles(n_fft);
    const int K = n_fft / 2 + 1;
    double* spec = new double[2 * (size_t)K];
    expect(ctx, "alsep_master_spectrum", alsep_master_spectrum(ctx, ms, n, n, p, pieces.data(), (int)pieces.size(), n_fft, 1.3, tw, spec, ws, wsb));
    finite("spectrum", spec, 2 * K);
    double* fir = track(2 * (int64_t)n_fft, 1.0);
    const int64_t cb = alsep_master_convolve_workspace_bytes(n_fft, log2_block, blocks_per_batch);
    char* cws = new char[(size_t)cb];
    double* conv = new double[2 * (size_t)n];
    expect(ctx, "alsep_master_convolve_same", alsep_master_convolve_same(ctx, ms, 2, n, n, fir, n_fft, 1.1, log2_block, conv, n, cws, cb));
    finite("convolution", conv, 2 * n);
    double* out = new double[2 * (size_t)n];
    expect(ctx, "alsep_master_leftright", alsep_master_leftright(ctx, conv, n, n, 1.2, out, n));
    std::printf("analysis: %lld samples, %d pieces of %lld, n_fft %d, block 2^%d: peak %.4f\n", (long long)n, d, (long long)p, n_fft, log2_block, peak[0]);
    delete[] ws; delete[] lr; delete[] ms; delete[] peak; delete[] sums; delete[] tw; delete[] spec; delete[] fir; delete[] cws; delete[] conv; delete[] out;
}

void convolution(alsep_ctx* ctx, int64_t n, int64_t taps, int log2_block, int blocks_per_batch) {
    double* x = track(n, 1.0);
    double* fir = track(taps, 1.0);
    double* y = new double[(size_t)n];
    const int64_t cb = alsep_master_convolve_workspace_bytes(taps, log2_block, blocks_per_batch);
    char* cws = new char[(size_t)cb];
    expect(ctx, "alsep_master_convolve_same", alsep_master_convolve_same(ctx, x, 1, n, n, fir, taps, 1.0, log2_block, y, n, cws, cb));
    finite("convolution", y, n);
    delete[] x; delete[] fir; delete[] y; delete[] cws;
}

void maxima(alsep_ctx* ctx, int64_t n, int w) {
    double* x = track(n, 1.0);
    double *a = new double[(size_t)n], *b = new double[(size_t)n];
    expect(ctx, "alsep_master_slide_max (centred)", alsep_master_slide_max(ctx, x, n, w, 1, a));
    expect(ctx, "alsep_master_slide_max (trailing)", alsep_master_slide_max(ctx, x, n, w, 0, b));
    for (int64_t i = 0; i < n; ++i) if (a[i] < x[i] || b[i] < x[i] || a[i] < b[i]) { std::printf("sliding maximum below its input at %lld\n", (long long)i); ++g_bad; break; }
    delete[] x; delete[] a; delete[] b;
}

void scans(alsep_ctx* ctx, int64_t n, int chunk, double a1) {
    double* x = track(n, 1.0);
    double* y = new double[(size_t)n];
    const int64_t ib = alsep_master_iir_workspace_bytes(n, chunk);
    char* iws = new char[(size_t)ib];
    expect(ctx, "alsep_master_iir", alsep_master_iir(ctx, x, n, 0.2, 0.1, a1, 0.3, 0, chunk, y, iws, ib));
    expect(ctx, "alsep_master_iir (reverse)", alsep_master_iir(ctx, x, n, 0.2, 0.1, a1, 0.3, 1, chunk, y, iws, ib));
    finite("iir", y, n);
    if (n > 6) {
        const int64_t fb = alsep_master_filtfilt_workspace_bytes(n, chunk);
        char* fws = new char[(size_t)fb];
        expect(ctx, "alsep_master_filtfilt", alsep_master_filtfilt(ctx, x, n, 1.0 + a1, 0.0, a1, -a1, chunk, y, fws, fb));
        finite("filtfilt", y, n);
        delete[] fws;
    }
    delete[] x; delete[] y; delete[] iws;
}

void limiter(alsep_ctx* ctx, int64_t n) {
    const int64_t wsb = alsep_master_workspace_bytes();
    char* ws = new char[(size_t)wsb];
    double* lr = track(2 * n, 3.0);
    double *g = new double[(size_t)n], *m = new double[(size_t)n], *gain = new double[(size_t)n], *peak = new double[1];
    int32_t* over = new int32_t[1];
    expect(ctx, "alsep_master_rectify", alsep_master_rectify(ctx, lr, n, n, 0.998, g, over));
    if (over[0] != 1) { std::printf("rectify: nothing above the threshold\n"); ++g_bad; }
    expect(ctx, "alsep_master_maximum", alsep_master_maximum(ctx, g, g, n, m));
    double *out = new double[2 * (size_t)n], *res = new double[2 * (size_t)n];
    expect(ctx, "alsep_master_limit_apply", alsep_master_limit_apply(ctx, lr, n, n, g, g, m, m, out, n, gain, peak, ws, wsb));
    expect(ctx, "alsep_master_limit_apply (no gain)", alsep_master_limit_apply(ctx, lr, n, n, g, g, m, m, out, n, nullptr, peak, ws, wsb));
    if (!(peak[0] <= 0.998 * (1 + 1e-12))) { std::printf("limit_apply: peak %.17g above the threshold\n", peak[0]); ++g_bad; }
    uint8_t* pcm = new uint8_t[6 * (size_t)n];
    expect(ctx, "alsep_master_pcm24", alsep_master_pcm24(ctx, out, n, n, 0.9, res, n, pcm));
    delete[] ws; delete[] lr; delete[] g; delete[] m; delete[] gain; delete[] peak; delete[] over; delete[] out; delete[] res; delete[] pcm;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    analysis(&ctx, 10007, 4, 2501, 256, 9, 2);
    analysis(&ctx, 12000, 5, 2400, 256, 12, 1);
    analysis(&ctx, 2999, 1, 2999, 256, 9, 64);
    analysis(&ctx, 256, 1, 256, 256, 9, 1);
    analysis(&ctx, 3 * 4096 + 5, 2, 6146, 4096, 13, 1);
    analysis(&ctx, 2 * 8192 + 1, 1, 2 * 8192 + 1, 8192, 14, 3);
    convolution(&ctx, 100, 256, 9, 1);
    convolution(&ctx, 257, 256, 9, 1);
    convolution(&ctx, 1000, 256, 9, 2);
    convolution(&ctx, 999, 255, 9, 3);
    maxima(&ctx, 89, 45);
    maxima(&ctx, 1000, 45);
    maxima(&ctx, 8189, 4095);
    maxima(&ctx, 20000, 4096);
    maxima(&ctx, 16385, 1);
    scans(&ctx, 200, 64, -0.95);
    scans(&ctx, 7, 0, -0.95);
    scans(&ctx, 7, 3, 0.6);
    scans(&ctx, 1, 0, -0.5);
    scans(&ctx, 40000, 0, -0.999962);
    scans(&ctx, 8193, 8192, -0.9);
    limiter(&ctx, 256);
    limiter(&ctx, 10007);
    // refused before any launch
    double* x = track(100, 1.0);
    double* y = new double[100];
    char* ws = new char[64];
    expect(&ctx, "slide_max with n < 2 w - 1", alsep_master_slide_max(&ctx, x, 88, 45, 1, y), ALSEP_ERR_ARG);
    expect(&ctx, "slide_max with a window above 8191", alsep_master_slide_max(&ctx, x, 100, 4097, 0, y), ALSEP_ERR_ARG);
    expect(&ctx, "filtfilt of 6 samples", alsep_master_filtfilt(&ctx, x, 6, 0.1, 0.0, -0.9, 0.9, 0, y, ws, 64), ALSEP_ERR_ARG);
    expect(&ctx, "iir with a small workspace", alsep_master_iir(&ctx, x, 100, 0.1, 0.0, -0.9, 0.0, 0, 8, y, ws, 64), ALSEP_ERR_ARG);
    expect(&ctx, "iir with a chunk above 8192", alsep_master_iir(&ctx, x, 100, 0.1, 0.0, -0.9, 0.0, 0, 8193, y, ws, 64), ALSEP_ERR_ARG);
    delete[] x; delete[] y; delete[] ws;
    std::printf(g_bad ? "FAILED\n" : "ok\n");
    return g_bad ? 1 : 0;
}
