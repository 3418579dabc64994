// ntt_lazy_arith.hip -- host program (own main, no HIP API call: runs without a GPU) for the lazy residue arithmetic of
// csrc/ntt_conv.hpp.  tests/test_ntt_arith_cpu.py builds it with hipcc and runs it.
//
// ntt_mul and ntt_red estimate a quotient by floor(x / P - 2^-10) and never correct it; the butterflies of ntt_reg_levels let
// magnitudes grow over seven levels.  Everything rests on the contract in the header: |a| < 2^39, 0 <= b < 2^32 (ntt_mul),
// |v| < 2^40 (ntt_red) -> an integer in [0, 2 P) congruent to the true value.  Random data practically never meets the inputs
// where the estimate could fail: a true remainder within a few units of 0 or of P at the top of the magnitude range.  This
// program goes there on purpose and compares with 128-bit integers, for both primes:
//   ntt_mul   a b = k and = P - k (mod P) for every k < 64 (b = k a^-1 mod P), |a| within 1e5 of 2^39 (below) and of 2^32 (either
//             side), both signs, b canonical and lifted by P where that stays below 2^32; then a few million random inputs
//   ntt_red   v = q P + r, r = k or P - k, for the q at the top of |v| < 2^40, around +-2^32 / P and around 0; random inputs
//   ntt_canon [0, 2 P) -> [0, P) at the edges
//   ntt_reg_levels<4, false> followed by <3, true> as ntt_lds_transform<7> runs them on one column (128 points): congruent to a
//             naive O(n^2) DFT with the tables of ntt_build_tables (forward and inverse), and the largest magnitude stays below
//             2^39 for worst-case inputs (all 2 P - 1 -- whose zero-frequency output 128 (2 P - 1) IS the largest a run of seven
//             levels can reach: every level's sums at most double --, alternating, random lazy residues)
// It also prints the largest power of two of |a| for which the adversarial family of ntt_mul still passes (the measured head
// room; a line "headroom_log2 N", not an assertion).  Exit status 0: every check passed.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
#include "ntt_conv.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

int g_fail = 0;
void fail(const char *what, int prime, double a, double b, double r) {
    if (g_fail++ < 20) std::printf("FAIL %s prime %d a %.1f b %.1f result %.3f\n", what, prime, a, b, r);
}

struct Rng {                                       // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
};

NttMod mod_of(uint32_t P) { NttMod md; md.P = (double)P; md.Pinv = 1.0 / (double)P; return md; }       // as ntt_setup fills it
uint32_t mod_i128(i128 x, uint32_t P) { i128 r = x % (i128)P; if (r < 0) r += P; return (uint32_t)r; }

// r is an integer in [0, 2 P) congruent to `want`
bool lazy_ok(double r, uint32_t want, uint32_t P) {
    if (!(r >= 0.0) || !(r < 2.0 * (double)P) || r != std::floor(r)) return false;
    return (uint32_t)((uint64_t)r % P) == want;
}
bool mul_ok(int64_t a, uint32_t b, uint32_t P, const NttMod md, double *res = nullptr) {
    const double r = ntt_mul((double)a, (double)b, md);
    if (res) *res = r;
    return lazy_ok(r, mod_i128((i128)a * (i128)b, P), P);
}

// the adversarial family at |a| = top - i, i < 1e5 in steps of 13 (top = 2^lg - 1), and, with `above`, at top + 1 + i as well:
// returns the number of inputs that failed
long long mul_family(int pi, int64_t top, bool above, bool report, long long *count) {
    const uint32_t P = NTT_PRIMES[pi];
    const NttMod md = mod_of(P);
    long long bad = 0, n = 0;
    for (int side = 0; side < (above ? 2 : 1); ++side)
        for (int64_t i = 0; i < 100000; i += 13) {
            const int64_t mag = side ? top + 1 + i : top - i;
            const uint32_t am = (uint32_t)(mag % P);
            if (!am) continue;
            const uint32_t inv = ntt_powmod(am, P - 2ull, P);
            for (int sign = 0; sign < 2; ++sign) {
                const int64_t a = sign ? -mag : mag;
                for (uint32_t k = 0; k < 64; ++k)
                    for (int hi = 0; hi < 2; ++hi) {
                        uint32_t target = hi ? (P - k) % P : k;                       // a b = target (mod P)
                        if (sign) target = (P - target) % P;                          // b is found for |a|
                        const uint32_t b = ntt_mulmod_u64(target, inv, P);
                        for (int lift = 0; lift < 2; ++lift) {
                            if (lift && (uint64_t)b + P >= (1ull << 32)) continue;
                            const uint32_t bb = lift ? b + P : b;
                            double r;
                            ++n;
                            if (!mul_ok(a, bb, P, md, &r)) { ++bad; if (report) fail("ntt_mul adversarial", pi, (double)a, (double)bb, r); }
                        }
                    }
            }
        }
    if (count) *count += n;
    return bad;
}

void check_mul(int pi) {
    const uint32_t P = NTT_PRIMES[pi];
    const NttMod md = mod_of(P);
    long long n = 0;
    mul_family(pi, (1ll << 39) - 1, false, true, &n);
    mul_family(pi, (1ll << 32) - 1, true, true, &n);
    Rng rng{0x5eed0000ull + pi};
    for (int i = 0; i < 3000000; ++i, ++n) {
        const uint64_t u = rng.next(), v = rng.next();
        const int lg = 1 + (int)(u % 39);                                             // magnitudes of every size up to 2^39 - 1
        int64_t a = (int64_t)((u >> 8) & ((1ull << lg) - 1));
        if (i % 8 == 0) a = (1ll << 39) - 1 - (int64_t)((u >> 8) & 0xffff);
        if (v & 1) a = -a;
        const uint32_t b = (uint32_t)(v >> 32);
        double r;
        if (!mul_ok(a, b, P, md, &r)) fail("ntt_mul random", pi, (double)a, (double)b, r);
    }
    // the corners themselves
    const int64_t as[] = {0, 1, -1, (1ll << 39) - 1, -((1ll << 39) - 1), (int64_t)P, -(int64_t)P, 2 * (int64_t)P - 1};
    const uint32_t bs[] = {0u, 1u, P - 1, P, P + 1, 2 * P - 1, 0xffffffffu};
    for (int64_t a : as) for (uint32_t b : bs) { double r; ++n; if (!mul_ok(a, b, P, md, &r)) fail("ntt_mul corner", pi, (double)a, (double)b, r); }
    std::printf("ntt_mul prime %u: %lld inputs\n", P, n);
}

void check_red(int pi) {
    const uint32_t P = NTT_PRIMES[pi];
    const NttMod md = mod_of(P);
    const int64_t lim = 1ll << 40;
    long long n = 0;
    auto one = [&](int64_t v, const char *what) {
        if (v <= -lim || v >= lim) return;
        ++n;
        const double r = ntt_red((double)v, md);
        if (!lazy_ok(r, mod_i128((i128)v, P), P)) fail(what, pi, (double)v, 0.0, r);
    };
    const int64_t qtop = lim / P, q32 = (1ll << 32) / P;
    std::vector<int64_t> qs;
    for (int64_t d = -3; d <= 3; ++d) { qs.push_back(d); qs.push_back(q32 + d); qs.push_back(-q32 + d); }
    for (int64_t d = 0; d <= 40; ++d) { qs.push_back(qtop + 1 - d); qs.push_back(-qtop - 2 + d); }
    for (int64_t q : qs)
        for (int64_t k = 0; k < 64; ++k) { one(q * P + k, "ntt_red adversarial"); one(q * P + P - k, "ntt_red adversarial"); one(q * P - k, "ntt_red adversarial"); }
    for (int64_t i = 0; i < 100000; ++i) { one(lim - 1 - i, "ntt_red top"); one(-(lim - 1 - i), "ntt_red top"); }
    Rng rng{0xabcd0000ull + pi};
    for (int i = 0; i < 3000000; ++i) {
        const uint64_t u = rng.next();
        const int lg = 1 + (int)(u % 40);
        int64_t v = (int64_t)((u >> 8) & ((1ull << lg) - 1));
        one((u >> 7) & 1 ? -v : v, "ntt_red random");
    }
    const uint32_t cs[] = {0u, 1u, P - 1, P, P + 1, 2 * P - 1};
    for (uint32_t c : cs) if (ntt_canon(c, P) != c % P) fail("ntt_canon", pi, (double)c, 0.0, (double)ntt_canon(c, P));
    std::printf("ntt_red prime %u: %lld inputs\n", P, n);
}

int brev7(int v) { int r = 0; for (int b = 0; b < 7; ++b) r |= ((v >> b) & 1) << (6 - b); return r; }

// one column of ntt_lds_transform<7>: pass 1 (rows n + 8 tt, four levels, no reduction), pass 2 (rows 8 u + v, three levels),
// ntt_red; slot s ends up holding frequency brev7(s).  *peak: the largest magnitude any pass left behind.
void transform128(double (&col)[128], const double *wtab, const NttMod md, double *peak) {
    for (int n = 0; n < 8; ++n) {
        double x[16];
        for (int tt = 0; tt < 16; ++tt) x[tt] = col[n + (tt << 3)];
        ntt_reg_levels<4, false>(x, wtab, n, 3, 0, md);
        for (int tt = 0; tt < 16; ++tt) { col[n + (tt << 3)] = x[tt]; *peak = std::max(*peak, std::fabs(x[tt])); }
    }
    for (int u = 0; u < 16; ++u) {
        double x[8];
        for (int v = 0; v < 8; ++v) x[v] = col[(u << 3) + v];
        ntt_reg_levels<3, true>(x, wtab, 0, 0, 4, md);
        for (int v = 0; v < 8; ++v) { *peak = std::max(*peak, std::fabs(x[v])); col[(u << 3) + v] = ntt_red(x[v], md); }
    }
}

void check_transform(int pi) {
    const uint32_t P = NTT_PRIMES[pi];
    const NttMod md = mod_of(P);
    double peak_all = 0.0;
    int runs = 0;
    for (int m : {14, 17, 21}) {                                   // (w_128 is the same root whatever m: the tables must say so)
        NttTables T;
        ntt_build_tables(m, P, NTT_ROOTS[pi], T);
        for (int inv = 0; inv < 2; ++inv) {
            double wtab[64];
            for (int j = 0; j < 64; ++j) wtab[j] = (double)T.wr[(size_t)inv * 192 + j];      // axis 0: w_128^(+-j)
            const uint32_t w1 = T.wr[(size_t)inv * 192 + 1];
            if (ntt_powmod(w1, 128, P) != 1u || ntt_powmod(w1, 64, P) != P - 1) fail("w_128 is not a primitive 128th root", pi, (double)w1, 0.0, 0.0);
            Rng rng{0x7777ull + 16 * m + 2 * pi + inv};
            for (int pattern = 0; pattern < 40; ++pattern, ++runs) {
                uint32_t in[128];
                for (int i = 0; i < 128; ++i) {
                    const uint32_t top = 2 * P - 1, rnd = (uint32_t)(rng.next() % (2ull * P));
                    in[i] = pattern == 0 ? top : pattern == 1 ? (i & 1 ? 0u : top) : pattern == 2 ? (i & 1 ? top : 0u) : pattern == 3 ? (i < 64 ? top : 0u)
                          : pattern == 4 ? (i & 2 ? P : top) : pattern == 5 ? (i == 0 ? top : 0u) : pattern < 12 ? (((i >> (pattern - 5)) & 1) ? top : 0u)
                          : pattern < 20 ? ((rnd & 1) ? top : (rnd & 2) ? P - 1 : 0u) : rnd;
                }
                double col[128], peak = 0.0;
                for (int i = 0; i < 128; ++i) col[i] = (double)in[i];
                transform128(col, wtab, md, &peak);
                peak_all = std::max(peak_all, peak);
                if (!(peak < 549755813888.0)) fail("magnitude reached 2^39", pi, peak, (double)pattern, 0.0);
                for (int k = 0; k < 128; ++k) {                   // naive DFT: X[k] = sum_i x[i] w^(i k)
                    uint64_t acc = 0;
                    const uint32_t wk = ntt_powmod(w1, (unsigned long long)k, P);
                    uint32_t cur = 1u;
                    for (int i = 0; i < 128; ++i) { acc = (acc + (uint64_t)ntt_mulmod_u64(in[i] % P, cur, P)) % P; cur = ntt_mulmod_u64(cur, wk, P); }
                    if (!lazy_ok(col[brev7(k)], (uint32_t)acc, P)) fail("transform", pi, (double)k, (double)pattern, col[brev7(k)]);
                }
            }
        }
    }
    std::printf("transform prime %u: %d columns, largest magnitude %.0f = 2^%.3f (limit 2^39)\n", P, runs, peak_all, std::log2(peak_all));
}
}  // namespace

int main() {
    for (int pi = 0; pi < 2; ++pi) { check_mul(pi); check_red(pi); check_transform(pi); }
    // head room: the adversarial family of ntt_mul at larger |a| (a b stays exact as h + l; only the quotient estimate can fail)
    int head = 0;
    for (int lg = 39; lg <= 52; ++lg) {
        long long bad = 0;
        for (int pi = 0; pi < 2; ++pi) bad += mul_family(pi, (1ll << lg) - 1, false, false, nullptr);
        std::printf("ntt_mul adversarial family below 2^%d: %lld failures\n", lg, bad);
        if (bad) break;
        head = lg;
    }
    std::printf("headroom_log2 %d\n", head);
    std::printf(g_fail ? "FAILED %d checks\n" : "PASS\n", g_fail);
    return g_fail ? 1 : 0;
}
