// TEST-ONLY, stand-alone: alsep_mix_sum / alsep_mix_power / alsep_mix_finish (csrc/mixdown.h through elementwise.hip, the unchanged kernel
// source on the CPU emulation) under AddressSanitizer.  Every buffer is a heap allocation of exactly the bytes the entry points are told
// about -- a mix of [channels][ld] holds (channels - 1) * ld + n elements -- so a kernel index one element outside any of them aborts the
// run.  Ragged stems (shorter and longer than the first, one mono), both widths, rows on and off the 16-byte grid, n = 1, stems chained
// over several launches; every integer is checked against a direct host computation.  Built and run by run_mixdown_asan.sh; nothing here
// is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "alsep_common.h"

namespace {

struct Geometry { const char* name; int channels; int64_t n; int64_t ld; int bits; int per_launch; std::vector<int64_t> stem_n; std::vector<int> stem_ch; };

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double noise() {                                                             // xorshift64*, uniform in (-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}
template <typename T> T* exact(size_t count) {                              // 16-byte aligned, not one byte more than asked for
    void* p = nullptr;
    if (posix_memalign(&p, 16, count * sizeof(T)) != 0) std::abort();
    return (T*)p;
}
int64_t clip(int64_t v, int64_t full) { return v < -full ? -full : v > full - 1 ? full - 1 : v; }
int64_t gain(int64_t a, double f, double full) { return (int64_t)std::floor(std::fmin(std::fmax((double)a * f, -full), full - 1.0)); }

int run(alsep_ctx* ctx, const Geometry& g) {
    const int64_t full = (int64_t)1 << (g.bits - 1);
    const size_t cells = (size_t)((g.channels - 1) * g.ld + g.n), k_stems = g.stem_n.size();
    std::vector<float*> data(k_stems);
    std::vector<alsep_mix_stem> stems(k_stems);
    std::vector<int64_t> want((size_t)(g.channels * g.n), 0);
    for (size_t k = 0; k < k_stems; ++k) {
        const int ch = g.stem_ch[k];
        const int64_t nk = g.stem_n[k];
        const int width = k == 1 ? 16 : g.bits;                              // one stem on the narrower grid, shifted up in a 32-bit mix
        data[k] = exact<float>((size_t)(ch * nk));
        for (int64_t i = 0; i < ch * nk; ++i) data[k][i] = (float)(0.6 * noise());
        stems[k] = {data[k], nk, nk, ch, width};
        const double scale = (double)((int64_t)1 << (width - 1));
        for (int c = 0; c < g.channels; ++c)
            for (int64_t i = 0; i < g.n && i < nk; ++i) {
                const double v = std::fmin(std::fmax(std::rint((double)data[k][(ch == 1 ? 0 : c) * nk + i] * scale), -scale), scale - 1.0);
                want[(size_t)(c * g.n + i)] = clip(want[(size_t)(c * g.n + i)] + (int64_t)v * ((int64_t)1 << (g.bits - width)), full);
            }
    }
    int32_t* acc = exact<int32_t>(cells);
    int32_t* out_i = exact<int32_t>(cells);
    float* out_f = exact<float>(cells);
    uint32_t* peak = exact<uint32_t>(1);
    int bad = 0;
    for (size_t first = 0; first < k_stems; first += (size_t)g.per_launch) {
        const int count = (int)std::min(k_stems - first, (size_t)g.per_launch);
        const int rc = alsep_mix_sum(ctx, first ? acc : nullptr, g.ld, stems.data() + first, count, g.channels, g.n, g.bits, acc, g.ld, peak);
        if (rc != ALSEP_OK) { std::printf("%s: alsep_mix_sum returned %d: %s\n", g.name, rc, ctx->err.c_str()); return 1; }
    }
    uint32_t want_peak = 0;
    for (int c = 0; c < g.channels; ++c)
        for (int64_t i = 0; i < g.n; ++i) {
            const int64_t w = want[(size_t)(c * g.n + i)];
            bad += acc[c * g.ld + i] != w;
            want_peak = std::max(want_peak, (uint32_t)(w < 0 ? -w : w));
        }
    bad += *peak != want_peak;
    const double f1 = 0.98 * (double)full / (double)(want_peak ? want_peak : 1), f2 = 0.3;
    const int64_t ws_bytes = alsep_mix_power_workspace_bytes(g.channels, g.n);
    char* ws = exact<char>((size_t)ws_bytes);
    uint64_t* pw = exact<uint64_t>(3);
    int rc = alsep_mix_power(ctx, acc, g.channels, g.n, g.ld, g.bits, f1, ws, ws_bytes, pw);
    if (rc == ALSEP_OK) rc = alsep_mix_finish(ctx, acc, g.channels, g.n, g.ld, g.bits, f1, f2, out_i, g.ld, out_f, g.ld);
    if (rc != ALSEP_OK) { std::printf("%s: power / finish returned %d: %s\n", g.name, rc, ctx->err.c_str()); return 1; }
    unsigned __int128 sum = 0;
    uint64_t peak1 = 0;
    for (int c = 0; c < g.channels; ++c)
        for (int64_t i = 0; i < g.n; ++i) {
            const int64_t y1 = gain(want[(size_t)(c * g.n + i)], f1, (double)full), y2 = gain(y1, f2, (double)full);
            sum += (unsigned __int128)(y1 * y1);
            peak1 = std::max(peak1, (uint64_t)(y1 < 0 ? -y1 : y1));
            bad += out_i[c * g.ld + i] != y2;
            bad += out_f[c * g.ld + i] != (float)((double)y2 / (double)full);
        }
    bad += pw[0] != peak1;
    bad += (((unsigned __int128)pw[1] << 32) + pw[2]) != sum;
    std::printf("%s: %d stems, %d per launch, peak %u: %d mismatches\n", g.name, (int)k_stems, g.per_launch, want_peak, bad);
    for (float* p : data) free(p);
    free(acc); free(out_i); free(out_f); free(peak); free(ws); free(pw);
    return bad ? 1 : 0;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    const Geometry cases[] = {
        {"ragged, aligned rows, 32 bit", 2, 1001, 1004, 32, 8, {1001, 700, 1500, 1001}, {2, 2, 2, 1}},
        {"ragged, dense odd rows, 32 bit", 2, 1001, 1001, 32, 8, {1001, 700, 1500, 1001}, {2, 2, 2, 1}},
        {"ragged, aligned rows, 16 bit", 2, 1001, 1004, 16, 8, {1001, 700, 1500, 1001}, {2, 2, 2, 1}},
        {"chained one by one", 2, 515, 516, 32, 1, {515, 3, 516, 600, 1}, {2, 2, 1, 2, 2}},
        {"chained two by two, dense", 3, 63, 63, 16, 2, {63, 61, 64, 63, 2}, {3, 1, 3, 3, 3}},
        {"one sample", 2, 1, 1, 32, 8, {1, 5, 1}, {2, 2, 1}},
        {"one sample, padded rows", 2, 1, 4, 16, 8, {1, 5, 1}, {2, 2, 1}},
        {"mono mix", 1, 777, 777, 32, 8, {777, 1000}, {1, 1}},
        {"several blocks", 2, 20001, 20004, 32, 8, {20001, 12000, 30000}, {2, 2, 1}},
    };
    int failed = 0;
    for (const Geometry& g : cases) failed += run(&ctx, g);
    std::printf(failed ? "FAILED\n" : "ok\n");
    return failed ? 1 : 0;
}
