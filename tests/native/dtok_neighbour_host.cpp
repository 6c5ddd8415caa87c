// The neighbour's verdict of the one-kernel SAM tokenizer (csrc/wk_dtok_neighbour.hpp) on the CPU: does a mapped line
// start a run, told from the five-word summaries of the line and of the line before it, against a plain byte compare of
// the whole QNAMEs.  Built and run by tests/test_dtok_neighbour_host.py with -fsanitize=address,undefined.  A summary
// is made the way the kernel makes it: from the two words that hold the line's first 16 bytes, whatever follows the
// QNAME in them (a tab, the FLAG, the next line) included.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "wk_dtok_neighbour.hpp"

namespace {

int g_checked = 0, g_failed = 0;

// the summary of a line that begins with `qname`, a tab and `rest`
wk::FnLine line_of(const std::string& qname, bool mapped, const std::string& rest = "99\tG000123\t1\t42\t50M") {
    const std::string text = qname + "\t" + rest + "\nnext\t0\tG1\n";
    unsigned char first[16] = {0};
    std::memcpy(first, text.data(), text.size() < 16 ? text.size() : 16);
    unsigned long long w0, w1;
    std::memcpy(&w0, first, 8);
    std::memcpy(&w1, first + 8, 8);
    return wk::fn_line(mapped, (uint32_t)qname.size(), w0, w1);
}

enum Want { kAny, kDecided };

// `cur` (mapped) behind `prev`: the verdict is never wrong, and where `want` says so it is a verdict
void check(const std::string& name, const std::string& prev, bool prev_mapped, bool prev_line, const std::string& cur, Want want) {
    ++g_checked;
    const wk::FnLine p = prev_line ? line_of(prev, prev_mapped, "0\tG7") : wk::fn_no_line(), c = line_of(cur, true);
    const wk::FnVerdict v = wk::fn_verdict(p, c);
    const bool same = prev == cur;  // the plain compare of whole QNAMEs
    const char* bad = nullptr;
    if (!prev_line || !prev_mapped) {
        if (v != wk::kFnUndecided) bad = "a line that is not behind a mapped line must be left undecided";
    } else if (v == wk::kFnStarts && same) {
        bad = "starts, but the QNAMEs are equal";
    } else if (v == wk::kFnContinues && !same) {
        bad = "continues, but the QNAMEs differ";
    } else if (v == wk::kFnUndecided) {
        // only QNAMEs of more than 16 bytes that agree in length and in their first 16 bytes
        if (cur.size() <= 16 || prev.size() != cur.size() || prev.compare(0, 16, cur, 0, 16) != 0) bad = "undecided, but length and first 16 bytes settle it";
        if (want == kDecided) bad = "undecided where a verdict was due";
    } else if (v != wk::kFnStarts && v != wk::kFnContinues) {
        bad = "no verdict at all";
    }
    if (bad && g_failed++ < 20) std::printf("FAIL %s: '%s' behind '%s': %s (verdict %u)\n", name.c_str(), cur.c_str(), prev.c_str(), bad, (unsigned)v);
}

std::string name_of(uint32_t n, uint32_t salt = 0) {
    std::string s(n, 'a');
    for (uint32_t i = 0; i < n; ++i) s[i] = (char)('A' + (i * 7u + salt) % 26u);
    return s;
}

}  // namespace

int main() {
    for (uint32_t n : {1u, 8u, 15u, 16u, 17u, 40u}) {
        const std::string q = name_of(n);
        const Want whole = n <= 16u ? kDecided : kAny;
        check("equal", q, true, true, q, whole);
        {
            std::string d = q;  // a difference at byte 0
            d[0] ^= 1;
            check("byte 0", d, true, true, q, kDecided);
        }
        if (n > 15u) {
            std::string d = q;  // ... at byte 15: the last that travels
            d[15] ^= 1;
            check("byte 15", d, true, true, q, kDecided);
        }
        if (n > 16u) {
            std::string d = q;  // ... at byte 16: the first that does not -- never "continues"
            d[16] ^= 1;
            ++g_checked;
            const wk::FnVerdict v = wk::fn_verdict(line_of(d, true), line_of(q, true));
            if (v != wk::kFnUndecided && g_failed++ < 20) std::printf("FAIL byte 16: length %u: verdict %u, not undecided\n", n, (unsigned)v);
            check("byte 16", d, true, true, q, kAny);
        }
        {
            std::string d = q;  // ... at the last byte
            d[n - 1u] ^= 1;
            check("last byte", d, true, true, q, n <= 16u ? kDecided : kAny);
        }
        // equal first 16 bytes (or all of the shorter one's), different lengths
        check("a byte longer", q + "x", true, true, q, kDecided);
        check("a byte shorter", q, true, true, q + "x", kDecided);
        if (n > 1u) check("a prefix", q.substr(0, n / 2u), true, true, q, kDecided);
        // what follows the QNAME in the 16 bytes is no part of it: a tab-and-FLAG tail that differs
        ++g_checked;
        if (n <= 16u && wk::fn_verdict(line_of(q, true, "0\tG1"), line_of(q, true, "147\tG2")) != wk::kFnContinues && g_failed++ < 20)
            std::printf("FAIL tail: length %u: equal QNAMEs, different FLAGs: not continues\n", n);
        check("predecessor unmapped", q, false, true, q, kAny);
        check("predecessor unmapped, another QNAME", name_of(n, 3), false, true, q, kAny);
        check("predecessor no line", "", false, false, q, kAny);
    }
    // every pair of lengths 1-40, equal up to the shorter; and random names over a two-letter alphabet
    for (uint32_t a = 1; a <= 40; ++a)
        for (uint32_t b = 1; b <= 40; ++b) check("lengths", name_of(a), true, true, name_of(b), a != b || a <= 16u ? kDecided : kAny);
    std::mt19937 rng(20240920);
    for (uint32_t r = 0; r < 20000; ++r) {
        const uint32_t n = 1u + rng() % 40u;
        std::string p(n, 'a'), c;
        for (auto& ch : p) ch = (char)('a' + rng() % 2u);
        c = p;
        if (rng() % 3u) c[rng() % n] = (char)('a' + rng() % 2u);
        if (rng() % 7u == 0) c.resize(1u + rng() % 40u, 'b');
        check("random", p, rng() % 9u != 0, rng() % 11u != 0, c, kAny);
    }
    std::printf("%d pairs checked, %d failures\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
