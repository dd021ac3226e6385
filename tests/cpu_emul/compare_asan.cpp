// TEST-ONLY, stand-alone: the Compare entry points (csrc/compare.h and alsep_resample_fft_f64 through reverb.hip, the unchanged kernel
// source on the CPU emulation) under AddressSanitizer.  Every buffer is a heap allocation of exactly the size the entry point is told,
// so a kernel index one element outside any of them aborts the run.  Shapes: the shortest track (2048 samples, 3 frames), a padded tail
// (2049), 5000 samples in launches of two frames, and the resampler's three paths -- 9601 -> 8820 (Bluestein both sides, going down),
// 8000 -> 8820 (going up) and 8192 -> 4096 (powers of two); the reductions with buckets that divide the length, that do not, and one
// sample / one frame per bucket.  Built and run by run_compare_asan.sh; nothing here is loaded into Python.
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

double* track(int64_t n) {
    double* x = new double[(size_t)n];
    for (int64_t i = 0; i < n; ++i) x[i] = 0.1 * noise() + 0.3 * std::sin(0.0627 * (double)i);
    return x;
}

int fail(alsep_ctx* ctx, const char* what, int rc) {
    std::printf("%s returned %d: %s\n", what, rc, ctx->err.c_str());
    return 1;
}

// x (n_in samples) -> a new array of n_out samples
int resampled(alsep_ctx* ctx, const double* x, int64_t n_in, int64_t n_out, double** out) {
    const int64_t need = alsep_resample_fft_f64_workspace_bytes(n_in, n_out);
    if (need < 0) return 1;
    char* ws = new char[(size_t)need];
    double* y = new double[(size_t)n_out];
    const int rc = alsep_resample_fft_f64(ctx, x, n_in, y, n_out, 1, n_in, n_out, ws, need);
    delete[] ws;
    *out = y;
    return rc != ALSEP_OK ? fail(ctx, "alsep_resample_fft_f64", rc) : 0;
}

int reductions(alsep_ctx* ctx, const double* w, int64_t n, const float* db, int64_t F) {
    int bad = 0;
    const int64_t ks[] = {1, 8, 613, n};
    for (int64_t K : ks) {
        if (K > n) continue;
        double *mn = new double[(size_t)K], *mx = new double[(size_t)K];
        int64_t *imn = new int64_t[(size_t)K], *imx = new int64_t[(size_t)K];
        const int rc = alsep_compare_minmax(ctx, w, n, K, mn, imn, mx, imx);
        if (rc != ALSEP_OK) bad += fail(ctx, "alsep_compare_minmax", rc);
        for (int64_t j = 0; j < K && !bad; ++j) {
            const int64_t lo = j * n / K, hi = (j + 1) * n / K;
            if (imn[j] < lo || imn[j] >= hi || imx[j] < lo || imx[j] >= hi || w[imn[j]] != mn[j] || w[imx[j]] != mx[j] || mn[j] > mx[j]) bad = 1;
        }
        delete[] mn; delete[] mx; delete[] imn; delete[] imx;
    }
    const int64_t kts[] = {1, 2, F};
    for (int64_t Kt : kts) {
        float* out = new float[(size_t)(1025 * Kt)];
        const int rc = alsep_compare_colmax(ctx, db, F, Kt, out);
        if (rc != ALSEP_OK) bad += fail(ctx, "alsep_compare_colmax", rc);
        if (Kt == F && std::memcmp(out, db, (size_t)(1025 * F) * sizeof(float)) != 0) bad = 1;
        delete[] out;
    }
    return bad;
}

// two tracks of na / nb samples, brought to ra / rb samples first (0: as they are), frames_per_batch frames per launch
int run(alsep_ctx* ctx, const char* name, int64_t na, int64_t ra, int64_t nb, int64_t rb, int frames_per_batch, const double* window,
        const double* twiddle) {
    double *a = track(na), *b = track(nb);
    int bad = 0;
    if (ra) { double* y = nullptr; bad += resampled(ctx, a, na, ra, &y); delete[] a; a = y; na = ra; }
    if (rb) { double* y = nullptr; bad += resampled(ctx, b, nb, rb, &y); delete[] b; b = y; nb = rb; }
    const int64_t n = na < nb ? na : nb, F = alsep_compare_frames(n);
    if (F < 0) bad = 1;
    if (!bad) {
        const int64_t ws_bytes = alsep_compare_rms_workspace_bytes();
        char* ws = new char[(size_t)ws_bytes];
        double* sumsq = new double[2];
        int rc = alsep_compare_rms(ctx, a, n, sumsq, ws, ws_bytes);
        if (rc == ALSEP_OK) rc = alsep_compare_rms(ctx, b, n, sumsq + 1, ws, ws_bytes);
        if (rc != ALSEP_OK) bad += fail(ctx, "alsep_compare_rms", rc);
        double *w0 = new double[(size_t)n], *w1 = new double[(size_t)n], *d = new double[(size_t)n];
        rc = alsep_compare_wave(ctx, a, b, n, sumsq, w0, w1, d);
        if (rc != ALSEP_OK) bad += fail(ctx, "alsep_compare_wave", rc);
        float *db1 = new float[(size_t)(1025 * F)], *db2 = new float[(size_t)(1025 * F)];
        double *l1 = new double[(size_t)(1025 * F)], *l2 = new double[(size_t)(1025 * F)];
        rc = alsep_compare_spectra(ctx, w0, w1, n, window, twiddle, frames_per_batch, db1, db2, l1, l2);
        if (rc == ALSEP_OK) rc = alsep_compare_spectra(ctx, w0, w1, n, window, twiddle, 0, db1, db2, nullptr, nullptr);   // as the wrapper calls it
        if (rc != ALSEP_OK) bad += fail(ctx, "alsep_compare_spectra", rc);
        double ms = 0.0, peak = 0.0;
        for (int64_t i = 0; i < n; ++i) ms += w0[i] * w0[i];
        for (int64_t i = 0; i < 1025 * F; ++i) {
            if (!std::isfinite(db1[i]) || !std::isfinite(db2[i]) || !std::isfinite(l1[i]) || !std::isfinite(l2[i])) bad = 1;
            peak = std::fmax(peak, l1[i]);
        }
        const double rms = std::sqrt(ms / (double)n);
        if (!(std::fabs(rms - 1.0) < 1e-12)) bad = 1;
        if (!bad) bad += reductions(ctx, w0, n, db1, F);
        std::printf("%s: %lld samples, %lld frames, rms of track 1 %.15f, peak of S1 %.4f: %s\n", name, (long long)n, (long long)F, rms, peak,
                    bad ? "BAD" : "ok");
        delete[] ws; delete[] sumsq; delete[] w0; delete[] w1; delete[] d; delete[] db1; delete[] db2; delete[] l1; delete[] l2;
    }
    delete[] a; delete[] b;
    return bad;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    const double pi = 3.14159265358979323846;
    double* window = new double[2048];
    double* twiddle = new double[2 * 2048];
    for (int m = 0; m < 2048; ++m) {
        window[m] = 0.5 - 0.5 * std::cos(2.0 * pi * m / 2048.0);
        twiddle[2 * m] = std::cos(2.0 * pi * m / 2048.0);
        twiddle[2 * m + 1] = -std::sin(2.0 * pi * m / 2048.0);
    }
    int bad = 0;
    bad += run(&ctx, "2048 samples", 2048, 0, 2048, 0, 0, window, twiddle);
    bad += run(&ctx, "2049 samples", 2049, 0, 2500, 0, 1, window, twiddle);
    bad += run(&ctx, "5000 samples, two frames per launch", 5000, 0, 5000, 0, 2, window, twiddle);
    bad += run(&ctx, "9600 / 9601 -> 8820", 9600, 8820, 9601, 8820, 0, window, twiddle);
    bad += run(&ctx, "8000 -> 8820, 8001 -> 8821", 8000, 8820, 8001, 8821, 3, window, twiddle);
    bad += run(&ctx, "8192 -> 4096", 8192, 4096, 4096, 0, 0, window, twiddle);
    // refused before any launch: too short, no buckets, more buckets than samples
    double* x = track(2047);
    float* out = new float[1];
    if (alsep_compare_spectra(&ctx, x, x, 2047, window, twiddle, 0, out, out, nullptr, nullptr) != ALSEP_ERR_ARG) bad += 1;
    if (alsep_compare_frames(2047) != -1) bad += 1;
    delete[] out; delete[] x; delete[] window; delete[] twiddle;
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
