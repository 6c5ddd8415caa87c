// The dealing of the one-kernel SAM tokenizer's line pass (csrc/wk_dtok_neighbour.hpp: fw_line, fw_has, fw_witness) on
// the CPU, against plain enumeration: lanes 1..63 of a wave own 63 consecutive lines, lane 0 is the witness
// of the line in front of them, a trip of eight waves covers 504 lines.  Built and run by
// tests/test_dtok_witness_host.py with -fsanitize=address,undefined.  The loop below is the kernel's:
//   for (k0 = first_line; k0 < n_lines; k0 += kFwTrip)  k = fw_line(k0, wave, lane), has = fw_has(k, first_line, n_lines)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wk_dtok_neighbour.hpp"

namespace {

int g_checked = 0, g_failed = 0;

void fail(uint32_t lines, uint32_t first_line, const char* what, long long at) {
    ++g_failed;
    std::printf("FAIL lines=%u first_line=%u at %lld: %s\n", lines, first_line, at, what);
}

constexpr long long kNoLine = -1;

// `lines` whole lines [first_line, first_line + lines)
void check(uint32_t lines, uint32_t first_line) {
    ++g_checked;
    const uint32_t n_lines = first_line + lines;
    std::vector<int> owners(n_lines, 0);
    uint32_t trips = 0;
    long long last_of_trip_before = kNoLine;  // thread 511's line of the trip before
    for (uint32_t k0 = first_line; k0 < n_lines; k0 += wk::kFwTrip, ++trips) {
        long long last_of_wave_before = last_of_trip_before;
        for (uint32_t wave = 0; wave < wk::kFwWaves; ++wave) {
            // what each lane of the wave holds: a line of the window, or none
            long long held[wk::kFwWave];
            for (uint32_t lane = 0; lane < wk::kFwWave; ++lane) {
                const uint32_t k = wk::fw_line(k0, wave, lane);
                held[lane] = wk::fw_has(k, first_line, n_lines) ? (long long)k : kNoLine;
                if (held[lane] != kNoLine && (k < first_line || k >= n_lines)) fail(lines, first_line, "a line outside the window", k);
            }
            if (!wk::fw_witness(0)) fail(lines, first_line, "lane 0 is no witness", wave);
            for (uint32_t lane = 1; lane < wk::kFwWave; ++lane) {
                if (wk::fw_witness(lane)) fail(lines, first_line, "a witness among the owners", lane);
                if (held[lane] == kNoLine) continue;
                ++owners[(size_t)held[lane]];
                // the lane below holds the line before; "no line" for the window's first line only
                const long long want = held[lane] == (long long)first_line ? kNoLine : held[lane] - 1;
                if (held[lane - 1] != want) fail(lines, first_line, "the lane below does not hold the line before", held[lane]);
            }
            // the witness: the last own line of the wave before, or of thread 511's wave in the trip before
            if (held[1] != kNoLine && held[1] != (long long)first_line && held[0] != last_of_wave_before)
                fail(lines, first_line, "the witness does not repeat the last own line of the wave before", held[1]);
            // owners are consecutive from lane 1 up: lines, then none
            for (uint32_t lane = 2; lane < wk::kFwWave; ++lane)
                if (held[lane] != kNoLine && held[lane - 1] == kNoLine) fail(lines, first_line, "a gap among a wave's owners", held[lane]);
            for (uint32_t lane = wk::kFwWave - 1u; lane >= 1u; --lane)
                if (held[lane] != kNoLine) {
                    last_of_wave_before = held[lane];
                    break;
                }
        }
        last_of_trip_before = last_of_wave_before;
    }
    for (uint32_t k = 0; k < n_lines; ++k) {
        const int want = k >= first_line ? 1 : 0;  // (the witness owns nothing: a line it alone holds has no owner)
        if (owners[k] != want) fail(lines, first_line, want ? "not exactly one owner" : "an owner of a line in front of the window's first", k);
    }
    if (trips != (lines + 503u) / 504u) fail(lines, first_line, "trips of the loop != ceil(lines / 504)", trips);
}

}  // namespace

int main() {
    static_assert(wk::kFwOwners == 63 && wk::kFwTrip == 504, "63 owners a wave, 504 lines a trip");
    const uint32_t sizes[] = {1, 62, 63, 64, 503, 504, 505, 1008, 1023};
    for (uint32_t lines : sizes)
        for (uint32_t first_line = 0; first_line < 2; ++first_line) check(lines, first_line);
    std::printf("dtok_witness_host: %d cases, %d failures\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
