// TEST-ONLY, stand-alone: the alsep_tempo_* entry points (csrc/tempo.h through reverb.hip, the unchanged kernel source on the CPU emulation)
// under AddressSanitizer.  Every buffer is a heap allocation of exactly the size the entry point is told, so a kernel index one element
// outside any of them aborts the run.  Geometries: one sample, fewer frames than the flux prefix, 2047 and 2049 samples, fewer frames than
// the tempogram window, an odd frame count above it; a filterbank whose last band ends on the last bin; the shortest and the longest
// period (15 and 515 offsets: one per lane at most, and nine).  Built and run by run_tempo_asan.sh; nothing here is loaded into Python.
#include <cmath>
#include <cstdio>

#include "alsep_common.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double noise() {                                                             // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

double* hann(int n) {
    double* w = new double[(size_t)n];
    for (int i = 0; i < n; ++i) w[i] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / n);
    return w;
}

int check(alsep_ctx* ctx, int rc, const char* what) {
    if (rc != ALSEP_OK) std::printf("%s returned %d: %s\n", what, rc, ctx->err.c_str());
    return rc != ALSEP_OK;
}

int finite(const double* v, int64_t n, const char* what) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) { std::printf("%s[%lld] is not finite\n", what, (long long)i); return 1; }
    return 0;
}

int run(alsep_ctx* ctx, int64_t n) {
    const int64_t F = alsep_tempo_frames(n);
    int bad = 0;
    double* y = new double[(size_t)n];
    for (int64_t i = 0; i < n; ++i) y[i] = 0.05 * noise() + ((i % 11025) < 400 ? std::sin(0.285 * (double)i) * std::exp(-(double)(i % 11025) / 80.0) : 0.0);
    double* win = hann(2048);
    double* tw = new double[2 * 2048];
    for (int m = 0; m < 2048; ++m) { tw[2 * m] = std::cos(2.0 * M_PI * m / 2048); tw[2 * m + 1] = -std::sin(2.0 * M_PI * m / 2048); }
    int32_t* bands = new int32_t[128 * 3];                                  // 9 bins each, 8 apart: band 127 ends on bin 1024
    const int64_t n_weights = 128 * 9;
    double* weights = new double[(size_t)n_weights];
    for (int b = 0; b < 128; ++b) { bands[3 * b] = 8 * b; bands[3 * b + 1] = 9; bands[3 * b + 2] = 9 * b; }
    for (int64_t i = 0; i < n_weights; ++i) weights[i] = 1.0 / 9.0;
    double* mel = new double[(size_t)(128 * F)];
    bad += check(ctx, alsep_tempo_mel(ctx, y, n, win, tw, bands, weights, n_weights, mel), "alsep_tempo_mel");
    bad += finite(mel, 128 * F, "mel");
    const int64_t flux_ws = alsep_tempo_flux_workspace_bytes(), tg_ws = alsep_tempo_tempogram_workspace_bytes();
    char* ws = new char[(size_t)flux_ws];
    double* db = new double[(size_t)(128 * F)];
    double* env = new double[(size_t)F];
    bad += check(ctx, alsep_tempo_flux(ctx, mel, F, db, env, ws, flux_ws), "alsep_tempo_flux");
    bad += finite(db, 128 * F, "db") + finite(env, F, "env");
    delete[] ws;
    double* stats = new double[3];
    bad += check(ctx, alsep_tempo_env_stats(ctx, env, F, stats), "alsep_tempo_env_stats");
    ws = new char[(size_t)tg_ws];
    double* win344 = hann(344);
    double* tg = new double[344];
    bad += check(ctx, alsep_tempo_tempogram(ctx, env, F, win344, tg, ws, tg_ws), "alsep_tempo_tempogram");
    bad += finite(tg, 344, "tg");
    delete[] ws;
    const bool flat = !(stats[0] > 0.0) || F < 2;                            // no tempo: the later stages would divide by a zero or NaN deviation
    for (int period : {9, 22, 64, 343}) {
        if (flat) break;
        double* gauss = new double[(size_t)(2 * period + 1)];
        for (int j = 0; j <= 2 * period; ++j) gauss[j] = std::exp(-0.5 * std::pow((j - period) * 32.0 / period, 2.0));
        double* ls = new double[(size_t)F];
        bad += check(ctx, alsep_tempo_local_score(ctx, env, F, stats, gauss, period, ls), "alsep_tempo_local_score");
        bad += finite(ls, F, "ls");
        const int w0 = -2 * period, count = 2 * period - (int)std::nearbyint(period / 2.0) + 1;
        double* txwt = new double[(size_t)count];
        for (int j = 0; j < count; ++j) txwt[j] = -100.0 * std::pow(std::log(-(double)(w0 + j) / period), 2.0);
        double* cum = new double[(size_t)F];
        int32_t* back = new int32_t[(size_t)F];
        bad += check(ctx, alsep_tempo_beat_dp(ctx, ls, F, txwt, w0, count, cum, back), "alsep_tempo_beat_dp");
        bad += finite(cum, F, "cum");
        for (int64_t i = 0; i < F; ++i)
            if (back[i] != -1 && (back[i] < i + w0 || back[i] > i + w0 + count - 1)) { std::printf("back[%lld] = %d\n", (long long)i, back[i]); bad += 1; break; }
        delete[] gauss; delete[] ls; delete[] txwt; delete[] cum; delete[] back;
    }
    std::printf("%lld samples, %lld frames: max|env| %.3g, std %.3g%s\n", (long long)n, (long long)F, stats[0], stats[2], bad ? " FAILED" : "");
    delete[] y; delete[] win; delete[] tw; delete[] bands; delete[] weights; delete[] mel; delete[] db; delete[] env; delete[] stats;
    delete[] win344; delete[] tg;
    return bad;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    int bad = 0;
    for (int64_t n : {(int64_t)1, (int64_t)1600, (int64_t)2047, (int64_t)2049, (int64_t)66150, (int64_t)200000}) bad += run(&ctx, n);
    // refusals come before any launch
    double in = 0.0, table[2] = {0.0, 0.0}, out = 0.0;
    int32_t b = 0;
    bad += alsep_tempo_frames(0) != -1 || alsep_tempo_frames((int64_t)3600 * 22050 + 1) != -1;
    bad += alsep_tempo_beat_dp(&ctx, &in, 1, table, -1, 2, &out, &b) == ALSEP_OK;              // an offset of 0
    bad += alsep_tempo_beat_dp(&ctx, &in, 1, table, -687, 1, &out, &b) == ALSEP_OK;            // beyond the ring
    bad += alsep_tempo_local_score(&ctx, &in, 1, table, table, 344, &out) == ALSEP_OK;         // a period above 343
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
