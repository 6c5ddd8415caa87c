// wk_dtok_rounds.hpp — how a window's 16-byte chunks are dealt to the waves of wk_dtok_fused.hpp.
//
// A window is kFrChunks = 1 280 chunks of text and one more behind them (below).  Every wave takes consecutive chunks
// -- so the newlines in front of a wave's chunks are the sum of the counts of the waves in front, and a wave numbers
// its own without a barrier -- in rounds of 64, a chunk per lane, and every round a wave runs is full: the first
// kFrLongWaves waves take three rounds (192 chunks), the others two (128).  Waves i and i + 4 share a SIMD: each SIMD
// runs five rounds.  Plain functions, the same on the host and on the device: tests/test_dtok_rounds_host.py holds
// them against a plain count on the CPU.
//
// The chunk behind the dealt ones (kFrTailChunk) is no wave's: a window looks at text positions [w0, w1) with
// w1 <= w0 + 16 * kFrChunks, the byte that stands for the newline of a text without a last one included (it lies in
// front of w1), so that chunk never holds text of the window.  It is what line offsets of 16 * kFrChunks point at
// and what loads that begin in the last dealt chunk run into: zeros, written once.
//
// The newlines of a wave's chunks travel round by round as fields of one 32-bit word, so that one scan over the lanes
// numbers all three rounds.  A field holds the running sum over the 64 chunks of a round.  A chunk of more than
// kFrChunkMax = 8 newlines has two of them next to each other -- an empty line, which has no three tabs: the block
// goes back to the six kernels (kDtokShortLine) whatever else it holds -- so the kernel raises that flag itself and
// counts no newline of such a chunk.  What is left is at most 8 x 64 = 512 per round, inside the 10 bits of a field
// at every lane of the scan: no field can carry into the next, and the counts of a block that is kept are exact.  (A
// window of 1 024 newlines or more is then seen as such -- its sum is exact -- and sets kDtokSpill as before.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WK_FR_FN __host__ __device__ __forceinline__
#else
#define WK_FR_FN inline
#endif

namespace wk {

constexpr uint32_t kFrWave = 64;                      // lanes: chunks of a round
constexpr uint32_t kFrWaves = 8;
constexpr uint32_t kFrLongWaves = 4;                  // waves of three rounds; the others run two
constexpr uint32_t kFrMaxRounds = 3;
constexpr uint32_t kFrChunks = (kFrLongWaves * 3u + (kFrWaves - kFrLongWaves) * 2u) * kFrWave;   // dealt chunks: 1 280
constexpr uint32_t kFrTailChunk = kFrChunks;          // the chunk behind them (see above)
constexpr uint32_t kFrChunkMax = 8;                   // newlines counted per chunk (more: an empty line)
constexpr uint32_t kFrNlBits = 10, kFrNlMask = (1u << kFrNlBits) - 1u;
static_assert(kFrChunkMax * kFrWave <= kFrNlMask, "a round's running sum fits its field");
static_assert(kFrMaxRounds * kFrNlBits <= 32u, "three fields in a word");

// rounds wave w runs, its chunks and the first of them
WK_FR_FN uint32_t fr_rounds(uint32_t w) { return w < kFrLongWaves ? 3u : 2u; }
WK_FR_FN uint32_t fr_chunks(uint32_t w) { return fr_rounds(w) * kFrWave; }
WK_FR_FN uint32_t fr_first_chunk(uint32_t w) {
    return w < kFrLongWaves ? w * 3u * kFrWave : kFrLongWaves * 3u * kFrWave + (w - kFrLongWaves) * 2u * kFrWave;
}

// Window limits in 32 bits.  min(base + len, lim) as 64-bit arithmetic gives it, for every 32-bit base, len and lim,
// without the 64-bit sum: where lim <= base the sum is the larger one (lim); where lim > base, lim - base does not wrap
// and "lim - base > len" says the same as "base + len < lim" -- and then the sum is below lim and does not wrap.
// Nothing is asked of the block's size.  (tests/test_dtok_limits32_host.py holds both against the 64-bit forms at the
// edges of the 32-bit range.)
WK_FR_FN uint32_t fr_min_end(uint32_t base, uint32_t len, uint32_t lim) { return lim > base && lim - base > len ? base + len : lim; }
// is base + len <= lim?  (lim - len does not wrap where lim >= len)
WK_FR_FN bool fr_fits(uint32_t base, uint32_t len, uint32_t lim) { return lim >= len && base <= lim - len; }

// the newlines of a chunk as they are counted: the mask, or none and `*blank` set where there are more than kFrChunkMax
WK_FR_FN uint32_t fr_chunk_marks(uint32_t marks16, bool* blank) {
    if ((uint32_t)__builtin_popcount(marks16) > kFrChunkMax) {
        *blank = true;
        return 0u;
    }
    return marks16;
}

// a round's count as its field of the word; the field of a word; the sum of a word's fields
WK_FR_FN uint32_t fr_pack(uint32_t count, uint32_t round) { return count << (kFrNlBits * round); }
WK_FR_FN uint32_t fr_unpack(uint32_t word, uint32_t round) { return (word >> (kFrNlBits * round)) & kFrNlMask; }
WK_FR_FN uint32_t fr_total(uint32_t word) { return fr_unpack(word, 0) + fr_unpack(word, 1) + fr_unpack(word, 2); }

}  // namespace wk
