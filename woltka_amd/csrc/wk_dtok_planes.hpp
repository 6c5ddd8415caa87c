// wk_dtok_planes.hpp — a window's owned lines as bit planes (wk_dtok_fused.hpp).
//
// Line k of the owned lines [ka, kb) is bit i % 64 of word i / 64, i = k - ka, of every plane: plane kFpStart has the
// lines that start a run, plane kFpFirst + m the first lines of their read (run, mate m) that name their subject.
// The bits at and behind kb - ka are clear.  A first line's position inside its read is the first lines of its mate
// from the head of its run up to itself, the read's size those up to the run's end: population counts over one or
// two words, where the kernel used to walk the lines' words.  Plain functions of a planes pointer and an index, the
// same on the host and on the device: tests/test_dtok_planes_host.py holds them against the walks on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WK_FP_FN __host__ __device__ __forceinline__
#else
#define WK_FP_FN inline
#endif

namespace wk {

constexpr uint32_t kFpMaxLines = 1280;               // kFzCarry + kFzLines
constexpr uint32_t kFpWords = kFpMaxLines / 64;      // words of a plane
constexpr uint32_t kFpStart = 0, kFpFirst = 1;       // planes: run starts; first lines of mate 0, 1, 2 (and 3: both mate bits)
constexpr uint32_t kFpPlanes = 5;

// bits 0..b of a word (b < 64): no shift by 64 at b = 63
WK_FP_FN unsigned long long fp_upto(uint32_t b) { return ~0ull >> (63u - b); }

// the head of line i's run: the highest set bit of `s` at or below i.  (One is set: the first owned line starts a run.)
WK_FP_FN uint32_t fp_head(const unsigned long long* s, uint32_t i) {
    uint32_t w = i >> 6;
    unsigned long long m = s[w] & fp_upto(i & 63u);
    while (m == 0ull && w > 0u) m = s[--w];
    return m ? w * 64u + 63u - (uint32_t)__builtin_clzll(m) : 0u;
}

// the end of line i's run: the lowest set bit of `s` above i, or n (the owned lines' number; i < n)
WK_FP_FN uint32_t fp_end(const unsigned long long* s, uint32_t i, uint32_t n) {
    const uint32_t words = (n + 63u) >> 6;
    uint32_t w = i >> 6;
    unsigned long long m = s[w] & ~fp_upto(i & 63u);
    while (m == 0ull && ++w < words) m = s[w];
    if (m == 0ull) return n;
    const uint32_t e = w * 64u + (uint32_t)__builtin_ctzll(m);
    return e < n ? e : n;
}

// the set bits of plane `f` in [lo, hi)
WK_FP_FN uint32_t fp_count(const unsigned long long* f, uint32_t lo, uint32_t hi) {
    uint32_t c = 0u;
    if (lo >= hi) return c;
    const uint32_t last = hi - 1u;
    for (uint32_t w = lo >> 6;; ++w) {  // (one word, mostly)
        unsigned long long m = f[w];
        if (w == lo >> 6) m &= ~0ull << (lo & 63u);
        if (w == last >> 6) m &= fp_upto(last & 63u);
        c += (uint32_t)__builtin_popcountll(m);
        if (w == last >> 6) return c;
    }
}

// What the kernel's records loop asks for first line i of mate plane `f` (n owned lines): the head of its run, its
// position among the read's first lines and the read's size.
struct FpRead {
    uint32_t head, pos, size;
};
WK_FP_FN FpRead fp_read(const unsigned long long* s, const unsigned long long* f, uint32_t i, uint32_t n) {
    FpRead r;
    r.head = fp_head(s, i);
    r.pos = fp_count(f, r.head, i);
    r.size = r.pos + fp_count(f, i, fp_end(s, i, n));
    return r;
}

}  // namespace wk
