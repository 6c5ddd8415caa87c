// The dealing of a window's chunks to the waves of the one-kernel SAM tokenizer (csrc/wk_dtok_rounds.hpp) on the CPU:
// every chunk dealt once and in order, the packed round counts against plain numbers, and the kernel's way to a
// window's newline total -- a chunk's marks, a round's field, a scan over the lanes, the sum of the last lane's
// fields, wave by wave -- against a plain count on random masks.  Built and run by tests/test_dtok_rounds_host.py with
// -fsanitize=address,undefined: the lists are heap arrays of exactly the chunks a case has.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "wk_dtok_rounds.hpp"

namespace {

int g_checked = 0, g_failed = 0;

void expect(bool ok, const std::string& what, long long got, long long want) {
    ++g_checked;
    if (!ok && g_failed++ < 20) std::printf("FAIL %s: %lld, expected %lld\n", what.c_str(), got, want);
}

// chunks 0 to kFrTailChunk once each and in order: the waves' rounds lane by lane, then the chunk that is no wave's
void check_dealing() {
    std::vector<uint32_t> seen;
    for (uint32_t w = 0; w < wk::kFrWaves; ++w) {
        expect(wk::fr_rounds(w) >= 1u && wk::fr_rounds(w) <= wk::kFrMaxRounds, "rounds of wave " + std::to_string(w), wk::fr_rounds(w), 3);
        expect(wk::fr_chunks(w) == wk::fr_rounds(w) * wk::kFrWave, "full rounds of wave " + std::to_string(w), wk::fr_chunks(w),
               wk::fr_rounds(w) * wk::kFrWave);
        for (uint32_t r = 0; r < wk::fr_rounds(w); ++r)
            for (uint32_t lane = 0; lane < wk::kFrWave; ++lane) seen.push_back(wk::fr_first_chunk(w) + r * wk::kFrWave + lane);
    }
    expect(seen.size() == wk::kFrChunks, "dealt chunks", (long long)seen.size(), wk::kFrChunks);
    seen.push_back(wk::kFrTailChunk);
    expect(seen.size() == 1281u, "chunks of a window", (long long)seen.size(), 1281);
    for (size_t i = 0; i < seen.size(); ++i) expect(seen[i] == i, "chunk at place " + std::to_string(i), seen[i], (long long)i);
    // (the seams the GPU test aims at, and the load of a SIMD: waves i and i + 4)
    expect(wk::fr_first_chunk(1) == 192u, "first chunk of wave 1", wk::fr_first_chunk(1), 192);
    expect(wk::fr_first_chunk(4) == 768u, "first chunk of wave 4", wk::fr_first_chunk(4), 768);
    expect(wk::fr_first_chunk(7) + wk::fr_chunks(7) == 1280u, "end of wave 7", wk::fr_first_chunk(7) + wk::fr_chunks(7), 1280);
    for (uint32_t i = 0; i < 4u; ++i) expect(wk::fr_rounds(i) + wk::fr_rounds(i + 4u) == 5u, "rounds of SIMD " + std::to_string(i), wk::fr_rounds(i) + wk::fr_rounds(i + 4u), 5);
}

// a count in every field, alone and with the other fields at their largest: what comes out is what went in
void check_pack() {
    const uint32_t largest = wk::kFrChunkMax * wk::kFrWave;  // (of a round of a window that is kept: 8 x 64)
    const uint32_t counts[] = {0u, 1u, 8u * 64u, largest, 511u, 2u};
    for (uint32_t c : counts)
        for (uint32_t r = 0; r < wk::kFrMaxRounds; ++r) {
            const uint32_t alone = wk::fr_pack(c, r);
            expect(wk::fr_unpack(alone, r) == c, "unpack alone", wk::fr_unpack(alone, r), c);
            expect(wk::fr_total(alone) == c, "total alone", wk::fr_total(alone), c);
            uint32_t word = alone;
            for (uint32_t o = 0; o < wk::kFrMaxRounds; ++o)
                if (o != r) word |= wk::fr_pack(largest, o);
            expect(wk::fr_unpack(word, r) == c, "unpack among full fields", wk::fr_unpack(word, r), c);
            for (uint32_t o = 0; o < wk::kFrMaxRounds; ++o)
                if (o != r) expect(wk::fr_unpack(word, o) == largest, "the field next to it", wk::fr_unpack(word, o), largest);
            expect(wk::fr_total(word) == c + 2u * largest, "total", wk::fr_total(word), c + 2u * largest);
        }
    // the words of 64 lanes added up (the scan's last lane) carry nothing from field to field
    uint32_t sum = 0;
    for (uint32_t lane = 0; lane < wk::kFrWave; ++lane)
        sum += wk::fr_pack(wk::kFrChunkMax, 0) | wk::fr_pack(wk::kFrChunkMax, 1) | wk::fr_pack(wk::kFrChunkMax, 2);
    for (uint32_t r = 0; r < wk::kFrMaxRounds; ++r) expect(wk::fr_unpack(sum, r) == largest, "a wave of full chunks", wk::fr_unpack(sum, r), largest);
    bool blank = false;
    expect(wk::fr_chunk_marks(0x00FFu, &blank) == 0x00FFu && !blank, "eight newlines are counted", blank, 0);
    expect(wk::fr_chunk_marks(0x01FFu, &blank) == 0u && blank, "nine are an empty line", blank, 1);
    blank = false;
    expect(wk::fr_chunk_marks(0xFFFFu, &blank) == 0u && blank, "sixteen too", blank, 1);
}

// The window's newlines the kernel's way against a plain count.  `marks`: a 16-bit mask per dealt chunk.
void check_sum(const std::string& name, const std::vector<uint32_t>& marks) {
    uint32_t plain = 0;
    bool plain_blank = false;
    for (uint32_t m : marks) {
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        if (c > wk::kFrChunkMax)
            plain_blank = true;
        else
            plain += c;
    }
    std::vector<uint32_t> wtot(wk::kFrWaves, 0u);
    std::vector<uint32_t> numbered;  // the number in front of every chunk, in chunk order
    bool blank = false;
    for (uint32_t w = 0; w < wk::kFrWaves; ++w) {
        std::vector<uint32_t> inc(wk::kFrWave, 0u);  // the scan: lane by lane
        for (uint32_t lane = 0; lane < wk::kFrWave; ++lane) {
            uint32_t packed = 0;
            for (uint32_t r = 0; r < wk::fr_rounds(w); ++r) {
                const uint32_t m = wk::fr_chunk_marks(marks.at(wk::fr_first_chunk(w) + r * wk::kFrWave + lane), &blank);
                packed |= wk::fr_pack((uint32_t)__builtin_popcount(m), r);
            }
            inc[lane] = (lane ? inc[lane - 1u] : 0u) + packed;
        }
        wtot[w] = wk::fr_total(inc[wk::kFrWave - 1u]);
        // (the number of a chunk's first newline as the kernel has it: the waves in front, the rounds in front, the lanes in front)
        uint32_t before = 0;
        for (uint32_t v = 0; v < w; ++v) before += wtot[v];
        uint32_t line = before;
        for (uint32_t r = 0; r < wk::fr_rounds(w); ++r) {
            for (uint32_t lane = 0; lane < wk::kFrWave; ++lane) {
                bool b2 = false;
                const uint32_t own = (uint32_t)__builtin_popcount(wk::fr_chunk_marks(marks.at(wk::fr_first_chunk(w) + r * wk::kFrWave + lane), &b2));
                numbered.push_back(line + wk::fr_unpack(inc[lane], r) - own);
            }
            line += wk::fr_unpack(inc[wk::kFrWave - 1u], r);
        }
    }
    uint32_t total = 0;
    for (uint32_t t : wtot) total += t;
    expect(total == plain, name + ": newlines of the window", total, plain);
    expect(blank == plain_blank, name + ": an empty line seen", blank, plain_blank);
    uint32_t run = 0;
    bool in_order = numbered.size() == marks.size();
    for (size_t c = 0; in_order && c < marks.size(); ++c) {
        in_order = numbered[c] == run;
        const uint32_t k = (uint32_t)__builtin_popcount(marks[c]);
        run += k > wk::kFrChunkMax ? 0u : k;
    }
    expect(in_order, name + ": every chunk's first line number", in_order, 1);
}

}  // namespace

int main() {
    check_dealing();
    check_pack();
    std::mt19937 rng(20240611u);
    check_sum("empty", std::vector<uint32_t>(wk::kFrChunks, 0u));
    check_sum("eight everywhere", std::vector<uint32_t>(wk::kFrChunks, 0x5555u));
    check_sum("one everywhere", std::vector<uint32_t>(wk::kFrChunks, 0x8000u));
    {
        std::vector<uint32_t> m(wk::kFrChunks, 0u);  // (the seams: the last chunk of a wave, the first of the next)
        for (uint32_t c : {0u, 63u, 64u, 191u, 192u, 767u, 768u, 895u, 896u, 1279u}) m[c] = 0x8001u;
        check_sum("seams", m);
        m[500] = 0x01FFu;  // (nine newlines: dropped and reported)
        check_sum("seams and a blank", m);
    }
    for (int t = 0; t < 300; ++t) {
        std::vector<uint32_t> m(wk::kFrChunks);
        const uint32_t density = 1u + rng() % 12u;  // (sixteenths: sparse windows, and windows of many blanks)
        for (auto& x : m) {
            x = 0u;
            for (uint32_t b = 0; b < 16u; ++b)
                if (rng() % 16u < density) x |= 1u << b;
        }
        check_sum("random " + std::to_string(t), m);
    }
    std::printf("dtok_rounds_host: %d checks, %d failures\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
