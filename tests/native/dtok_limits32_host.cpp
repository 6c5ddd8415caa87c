// The window limits of the one-kernel SAM tokenizer in 32 bits (csrc/wk_dtok_rounds.hpp: fr_min_end, fr_fits) against
// the 64-bit arithmetic they replace, on the CPU.  The kernel computed min(base + len, lim) and base + len <= lim with
// 64-bit sums; the 32-bit forms must say the same for EVERY 32-bit base, len and lim -- nothing is asked of the size
// of the block, so the cases that matter are the ones no GPU test can hold: positions next to 2^32.  Here: every
// combination of values at the edges of the range (0, 1, the kernel's window sizes and their neighbours, 2^31 and
// 2^32 less those), and random triples.  Built and run by tests/test_dtok_limits32_host.py with
// -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "wk_dtok_rounds.hpp"

namespace {

long long g_checked = 0, g_failed = 0;

void check(uint32_t base, uint32_t len, uint32_t lim) {
    const uint64_t sum = (uint64_t)base + len;
    const uint32_t want_end = (uint32_t)std::min<uint64_t>(sum, lim);  // (at most lim: fits)
    const bool want_fits = sum <= (uint64_t)lim;
    ++g_checked;
    if (wk::fr_min_end(base, len, lim) != want_end && g_failed++ < 20)
        std::printf("FAIL fr_min_end(%u, %u, %u) = %u, expected %u\n", base, len, lim, wk::fr_min_end(base, len, lim), want_end);
    ++g_checked;
    if (wk::fr_fits(base, len, lim) != want_fits && g_failed++ < 20)
        std::printf("FAIL fr_fits(%u, %u, %u) = %d, expected %d\n", base, len, lim, (int)wk::fr_fits(base, len, lim), (int)want_fits);
}

}  // namespace

int main() {
    // the kernel's lengths: kFzFwd, kFzTile + kFzFwd, kFzWin, a round of a wave
    const uint32_t lens[] = {0u, 1u, 16u, 1024u, 3072u, 16384u + 3072u, 20480u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    std::vector<uint32_t> edge;
    for (uint32_t c : {0u, 0x80000000u}) {
        for (uint32_t d = 0; d < 3; ++d) {
            edge.push_back(c + d);
            edge.push_back(c - 1u - d);  // (0 - 1 - d: the top of the range)
        }
        for (uint32_t l : lens)
            for (int d = -1; d <= 1; ++d) {
                edge.push_back(c + l + (uint32_t)d);
                edge.push_back(c - l + (uint32_t)d);
            }
    }
    std::sort(edge.begin(), edge.end());
    edge.erase(std::unique(edge.begin(), edge.end()), edge.end());
    for (uint32_t base : edge)
        for (uint32_t len : edge)
            for (uint32_t lim : edge) check(base, len, lim);
    std::mt19937_64 rng(15);
    for (int i = 0; i < 2000000; ++i) {
        const uint64_t r = rng();
        const uint32_t base = (uint32_t)r, lim = (uint32_t)(r >> 32);
        check(base, lens[i % 10], lim);
        check(base, lens[i % 10], base + (uint32_t)(rng() % 40000u));  // (a limit a window's length away: may wrap)
        check(base, (uint32_t)rng(), lim);
    }
    std::printf("%lld checks, %lld failures\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
