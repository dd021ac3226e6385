// TEST-ONLY, stand-alone: alsep_mix_sum_rates / alsep_mix_ratecv_length (csrc/mixdown.h through elementwise.hip, the unchanged kernel source
// on the CPU emulation) under AddressSanitizer.  Every buffer is a heap allocation of exactly the bytes the entry points are told about
// -- [channels][ld] holds (channels - 1) * ld + n elements -- so a kernel index one element outside any of them aborts the run: the
// interpolation reads x[j - 1] and x[j] with j up to n - 1, and nothing else.  Odd lengths, N = 1, 24-fold down and up, rows on and off
// the 16-byte grid, a mono stem, a 16-bit stem in a 32-bit mix, a resampled running mix (prev) with stems behind it; every integer is
// checked against a direct host loop that walks audioop.ratecv's own recurrence.  Built and run by run_mix_rate_asan.sh; nothing here is
// loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "alsep_common.h"

namespace {

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
int64_t gcd(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// audioop.ratecv with weightA = 1, weightB = 0 and no state, one channel: its two loops as they stand in the C module
std::vector<int64_t> ratecv(const std::vector<int64_t>& u, int width, int64_t in_rate, int64_t out_rate) {
    if (in_rate == out_rate) return u;
    const int64_t g = gcd(in_rate, out_rate), inr = in_rate / g, outr = out_rate / g;
    const int sh = 32 - width;
    std::vector<int64_t> out;
    int64_t d = -outr, prev = 0, cur = 0;
    size_t next = 0;
    for (;;) {
        while (d < 0) {
            if (next == u.size()) return out;
            prev = cur;
            cur = u[next++] * ((int64_t)1 << sh);
            d += outr;
        }
        while (d >= 0) {
            const int o = (int)(((double)prev * (double)d + (double)cur * (double)(outr - d)) / (double)outr);
            out.push_back((int64_t)(o >> sh));
            d -= inr;
        }
    }
}

struct Stem { int channels; int64_t n; int width; int64_t rate; };
struct Geometry {
    const char* name; int channels; int bits; bool dense;                   // dense: row stride = row length (off the 16-byte grid when odd)
    int64_t mix_n, mix_rate; int mix_width;                                  // mix_n > 0: operand 0 is a running mix of that length and rate
    int64_t rate;                                                            // the rate of the result
    std::vector<Stem> stems;
};

int64_t stride_of(int64_t n, bool dense) { return dense ? n : (n + 3) / 4 * 4; }

int run(alsep_ctx* ctx, const Geometry& g) {
    const int64_t full = (int64_t)1 << (g.bits - 1);
    std::vector<alsep_mix_operand> ops;
    std::vector<void*> owned;
    std::vector<std::vector<int64_t>> want((size_t)g.channels);              // per channel, grows to n_out with the first operand
    int64_t n_out = -1;
    auto add = [&](int c, const std::vector<int64_t>& v, int up_shift) {
        if (n_out < 0) want[(size_t)c].assign(v.size(), 0);
        std::vector<int64_t>& w = want[(size_t)c];
        for (size_t i = 0; i < w.size() && i < v.size(); ++i) w[i] = clip(w[i] + v[i] * ((int64_t)1 << up_shift), full);
    };
    if (g.mix_n > 0) {
        const int64_t ld = stride_of(g.mix_n, g.dense);
        int32_t* mix = exact<int32_t>((size_t)((g.channels - 1) * ld + g.mix_n));
        owned.push_back(mix);
        for (int c = 0; c < g.channels; ++c) {
            std::vector<int64_t> u((size_t)g.mix_n);
            for (int64_t i = 0; i < g.mix_n; ++i) {
                int64_t v = clip((int64_t)std::llrint(1.3 * noise() * (double)full), full);          // some samples sit on the clip values
                v = (v >> (g.bits - g.mix_width)) * ((int64_t)1 << (g.bits - g.mix_width));          // a mix of stems of that width
                mix[c * ld + i] = (int32_t)v;
                u[(size_t)i] = v >> (g.bits - g.mix_width);
            }
            add(c, ratecv(u, g.mix_width, g.mix_rate, g.rate), g.bits - g.mix_width);
        }
        n_out = (int64_t)want[0].size();
        ops.push_back({mix, g.mix_n, ld, g.mix_rate, g.rate, g.channels, g.mix_rate == g.rate ? g.bits : g.mix_width, 1});
    }
    for (const Stem& s : g.stems) {
        const int64_t ld = stride_of(s.n, g.dense);
        float* x = exact<float>((size_t)((s.channels - 1) * ld + s.n));
        owned.push_back(x);
        const double scale = (double)((int64_t)1 << (s.width - 1));
        std::vector<std::vector<int64_t>> res;
        for (int c = 0; c < s.channels; ++c) {
            std::vector<int64_t> u((size_t)s.n);
            for (int64_t i = 0; i < s.n; ++i) {
                x[c * ld + i] = (float)(1.1 * noise());                      // beyond +-1 now and then: the quantiser clips
                u[(size_t)i] = (int64_t)std::fmin(std::fmax(std::rint((double)x[c * ld + i] * scale), -scale), scale - 1.0);
            }
            res.push_back(ratecv(u, s.width, s.rate, g.rate));
        }
        for (int c = 0; c < g.channels; ++c) add(c, res[s.channels == 1 ? 0 : (size_t)c], g.bits - s.width);
        if (n_out < 0) n_out = (int64_t)want[0].size();
        ops.push_back({x, s.n, ld, s.rate == g.rate ? 0 : s.rate, s.rate == g.rate ? 0 : g.rate, s.channels, s.width, 0});
    }
    int bad = 0;
    const alsep_mix_operand& first = ops[0];
    bad += alsep_mix_ratecv_length(first.n, first.in_rate ? first.in_rate : 1, first.out_rate ? first.out_rate : 1) != n_out;
    const int64_t ld_acc = stride_of(n_out, g.dense);
    int32_t* acc = exact<int32_t>((size_t)((g.channels - 1) * ld_acc + n_out));
    uint32_t* peak = exact<uint32_t>(1);
    const int rc = alsep_mix_sum_rates(ctx, ops.data(), (int)ops.size(), g.channels, n_out, g.bits, acc, ld_acc, peak);
    if (rc != ALSEP_OK) { std::printf("%s: alsep_mix_sum_rates returned %d: %s\n", g.name, rc, ctx->err.c_str()); return 1; }
    uint32_t want_peak = 0;
    for (int c = 0; c < g.channels; ++c)
        for (int64_t i = 0; i < n_out; ++i) {
            const int64_t w = want[(size_t)c][(size_t)i];
            bad += acc[c * ld_acc + i] != w;
            want_peak = std::max(want_peak, (uint32_t)(w < 0 ? -w : w));
        }
    bad += *peak != want_peak;
    std::printf("%s: %d operands -> %d x %lld, peak %u: %d mismatches\n", g.name, (int)ops.size(), g.channels, (long long)n_out, want_peak, bad);
    for (void* p : owned) free(p);
    free(acc); free(peak);
    return bad ? 1 : 0;
}

int rejected(alsep_ctx* ctx) {
    int32_t* mix = exact<int32_t>(2 * 64);
    uint32_t* peak = exact<uint32_t>(1);
    const alsep_mix_operand alias = {mix, 40, 64, 44100, 48000, 2, 32, 1};   // resampled into its own rows
    const alsep_mix_operand rate0 = {mix, 40, 64, 0, 48000, 2, 32, 1};
    int32_t* acc = exact<int32_t>(2 * 64);
    int bad = 0;
    bad += alsep_mix_ratecv_length(40, 44100, 48000) != 43;                  // 39 * 160 / 147 + 1
    bad += alsep_mix_sum_rates(ctx, &alias, 1, 2, 43, 32, mix, 64, peak) != ALSEP_ERR_ARG;
    bad += alsep_mix_sum_rates(ctx, &rate0, 1, 2, 43, 32, acc, 64, peak) != ALSEP_ERR_ARG;
    bad += alsep_mix_sum_rates(ctx, &alias, 1, 2, 42, 32, acc, 64, peak) != ALSEP_ERR_ARG;   // not the length ratecv returns
    bad += alsep_mix_sum_rates(ctx, &alias, 1, 2, 44, 32, acc, 64, peak) != ALSEP_ERR_ARG;
    std::printf("rejected before any launch: %d wrong\n", bad);
    free(mix); free(peak); free(acc);
    return bad ? 1 : 0;
}

}  // namespace

int main() {
    alsep_ctx ctx;
    const Geometry cases[] = {
        {"one stem 44100 -> 48000, odd, aligned rows", 2, 32, false, 0, 0, 0, 48000, {{2, 1001, 32, 44100}}},
        {"one stem 48000 -> 44100, odd, dense rows", 2, 32, true, 0, 0, 0, 44100, {{2, 1001, 32, 48000}}},
        {"16 bit, 40000 -> 44100, dense", 2, 16, true, 0, 0, 0, 44100, {{2, 777, 16, 40000}}},
        {"one sample up", 2, 32, true, 0, 0, 0, 192000, {{2, 1, 32, 8000}}},
        {"one sample down", 1, 16, false, 0, 0, 0, 8000, {{1, 1, 16, 192000}}},
        {"24 times up", 2, 32, true, 0, 0, 0, 192000, {{2, 301, 32, 8000}}},
        {"24 times down", 2, 16, true, 0, 0, 0, 8000, {{2, 4099, 16, 192000}}},
        {"24 times down, fewer than 24 samples", 2, 32, false, 0, 0, 0, 8000, {{2, 23, 32, 192000}}},
        {"1048573 -> 1048576", 1, 32, true, 0, 0, 0, 1048576, {{1, 515, 32, 1048573}}},
        {"stems as they are and resampled, ragged, one mono, one 16 bit", 2, 32, false, 0, 0, 0, 48000,
         {{2, 1001, 32, 48000}, {2, 700, 32, 44100}, {1, 1500, 16, 40000}, {2, 63, 32, 48000}, {2, 3000, 32, 22050}}},
        {"the same, dense rows", 2, 32, true, 0, 0, 0, 48000,
         {{2, 1001, 32, 48000}, {2, 700, 32, 44100}, {1, 1500, 16, 40000}, {2, 63, 32, 48000}, {2, 3000, 32, 22050}}},
        {"a resampled mix, then stems", 2, 32, false, 1001, 44100, 32, 48000, {{2, 1200, 32, 48000}, {2, 500, 32, 44100}, {1, 900, 16, 48000}}},
        {"a resampled mix, dense rows", 2, 32, true, 1001, 44100, 32, 48000, {{2, 1200, 32, 48000}, {2, 500, 32, 44100}}},
        {"a 16-bit mix in a 32-bit container, resampled", 2, 32, false, 515, 44100, 16, 48000, {{2, 600, 32, 48000}}},
        {"a 16-bit mix, 24 times up, alone", 2, 16, true, 63, 8000, 16, 192000, {}},
        {"a one-sample mix", 2, 32, true, 1, 22050, 32, 44100, {{2, 5, 32, 44100}}},
        {"the mix as it is, seven stems", 2, 32, false, 1001, 48000, 32, 48000,
         {{2, 1001, 32, 44100}, {2, 1001, 32, 48000}, {2, 10, 32, 40000}, {1, 2000, 32, 48000}, {2, 999, 16, 32000}, {2, 1, 32, 8000}, {2, 1002, 32, 48000}}},
        {"several blocks", 2, 32, false, 0, 0, 0, 48000, {{2, 20001, 32, 44100}, {2, 30000, 32, 48000}, {1, 12000, 32, 40000}}},
    };
    int failed = rejected(&ctx);
    for (const Geometry& g : cases) failed += run(&ctx, g);
    std::printf(failed ? "FAILED\n" : "ok\n");
    return failed ? 1 : 0;
}
