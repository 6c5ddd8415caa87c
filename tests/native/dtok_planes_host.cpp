// The plane arithmetic of the one-kernel SAM tokenizer (csrc/wk_dtok_planes.hpp) on the CPU: head, end, position and
// size from the planes against the walks' definition written out plainly.  Built and run by
// tests/test_dtok_planes_host.py with -fsanitize=address,undefined: the planes are heap arrays of exactly the words a
// case has, so a word read past them or a shift by 64 ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "wk_dtok_planes.hpp"

namespace {

struct Lines {
    std::vector<uint8_t> start, first, mate;  // per owned line: starts a run; first line of its (run, mate); mate 0-3
    size_t n() const { return start.size(); }
    void add(bool s, bool f, uint32_t m) {
        start.push_back(s);
        first.push_back(f);
        mate.push_back((uint8_t)m);
    }
};

int g_checked = 0, g_failed = 0;

void fail(const std::string& name, size_t i, const char* what, uint32_t got, uint32_t want) {
    if (g_failed++ < 20) std::printf("FAIL %s: line %zu: %s %u, the walk gives %u\n", name.c_str(), i, what, got, want);
}

// What wk_dtok_fused.hpp's records loop used to walk: back from the line to the line that starts its run, counting
// the first lines of the line's mate in front of it; ahead to the next run start or the end of the owned lines.
void check(const std::string& name, const Lines& L) {
    const uint32_t n = (uint32_t)L.n();
    if (n) {
        if (n > wk::kFpMaxLines || !L.start[0]) {
            std::printf("FAIL %s: not a case (%u lines, first line starts %d)\n", name.c_str(), n, (int)L.start[0]);
            ++g_failed;
            return;
        }
    }
    const uint32_t words = (n + 63u) / 64u;
    std::vector<std::vector<unsigned long long>> planes(wk::kFpPlanes);
    for (auto& p : planes) p.assign(words, 0ull);  // (no word more than the lines need)
    for (uint32_t i = 0; i < n; ++i) {
        if (L.start[i]) planes[wk::kFpStart][i / 64u] |= 1ull << (i % 64u);
        if (L.first[i]) planes[wk::kFpFirst + L.mate[i]][i / 64u] |= 1ull << (i % 64u);
    }
    const unsigned long long* s = planes[wk::kFpStart].data();
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t h = i;
        while (!L.start[h]) --h;
        uint32_t e = i + 1u;
        while (e < n && !L.start[e]) ++e;
        const uint32_t gh = wk::fp_head(s, i), ge = wk::fp_end(s, i, n);
        if (gh != h) fail(name, i, "head", gh, h);
        if (ge != e) fail(name, i, "end", ge, e);
        for (uint32_t m = 0; m < 4u; ++m) {  // (every plane at every line: ranges that begin and end anywhere)
            uint32_t pos = 0, size = 0;
            for (uint32_t j = h; j < e; ++j) {
                const uint32_t one = L.first[j] && L.mate[j] == m ? 1u : 0u;
                if (j < i) pos += one;
                size += one;
            }
            const unsigned long long* f = planes[wk::kFpFirst + m].data();
            const uint32_t gp = wk::fp_count(f, gh, i), gs = wk::fp_count(f, gh, ge);
            if (gp != pos) fail(name, i, "count [head, line)", gp, pos);
            if (gs != size) fail(name, i, "count [head, end)", gs, size);
            if (L.first[i] && L.mate[i] == m) {
                const wk::FpRead r = wk::fp_read(s, f, i, n);
                if (r.head != h) fail(name, i, "read head", r.head, h);
                if (r.pos != pos) fail(name, i, "pos", r.pos, pos);
                if (r.size != size) fail(name, i, "size", r.size, size);
                ++g_checked;
            }
            if (wk::fp_count(f, i, i) != 0u) fail(name, i, "empty range", 1u, 0u);
        }
    }
    const unsigned long long none = 0ull;  // (an empty range reads nothing: n = 0 has no word at all)
    if (wk::fp_count(n ? planes[1].data() : &none, n, n) != 0u || wk::fp_count(&none, 0u, 0u) != 0u) fail(name, n, "empty range at the end", 1u, 0u);
}

// n lines with runs that start at line 0 and at `starts`; every `first_every`-th line and every run start is a first
// line, of mate (i * 7 / 3) % 3.
Lines from_starts(uint32_t n, const std::vector<uint32_t>& starts, uint32_t first_every = 1) {
    Lines L;
    for (uint32_t i = 0; i < n; ++i) {
        bool s = i == 0;
        for (uint32_t x : starts) s |= x == i;
        L.add(s, i % first_every == 0 || s, (i * 7u / 3u) % 3u);
    }
    return L;
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t rounds = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 300u;
    // hand-made
    check("head at bits 0 and 63", from_starts(256, {63, 64, 127, 128, 192}));
    check("end at the next word's bit 0", from_starts(200, {64, 128}));
    check("end at bit 63", from_starts(200, {63, 127, 191}, 2));
    check("a run over three whole words", from_starts(400, {10, 64, 256, 300}));
    check("a run over three whole words, few first lines", from_starts(400, {64, 256}, 37));
    for (uint32_t q : {1u, 2u, 8u, 20u}) {
        check("64q lines", from_starts(64u * q, {5}));
        if (q < 20u) check("64q + 1 lines", from_starts(64u * q + 1u, {64u * q - 1u}));
        if (q < 20u) check("64q + 1 lines, the last a run", from_starts(64u * q + 1u, {64u * q}));
        check("64q lines, one run", from_starts(64u * q, {}));
    }
    check("no lines", Lines());
    check("one line", from_starts(1, {}));
    check("a single-line run at 1279", from_starts(1280, {600, 1279}, 3));
    check("1280 lines, one run", from_starts(1280, {}));
    {
        Lines L;  // three mates, each its own pattern; and lines of both mate bits between them
        for (uint32_t i = 0; i < 700; ++i) {
            const uint32_t m = i % 11 == 0 ? 3u : (i % 5 < 2 ? 0u : (i % 5 < 3 ? 1u : 2u));
            L.add(i == 0 || i == 190 || i == 449, m == 0 ? i % 2 == 0 : (m == 1 ? i % 3 != 0 : true), m);
        }
        check("three mate planes", L);
    }
    {
        Lines L;  // every line starts a run
        for (uint32_t i = 0; i < 130; ++i) L.add(true, true, i % 3);
        check("runs of one line", L);
    }
    // random
    std::mt19937 rng(20240611);
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t n = 1u + rng() % wk::kFpMaxLines;
        const uint32_t run_len = 1u + rng() % (r % 3 == 0 ? 400u : 40u), first_pct = rng() % 101u;
        Lines L;
        for (uint32_t i = 0; i < n; ++i) L.add(i == 0 || rng() % run_len == 0, rng() % 100u < first_pct, rng() % (r % 5 == 0 ? 4u : 3u));
        check("random " + std::to_string(r), L);
    }
    std::printf("%d first lines checked, %d failures\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
