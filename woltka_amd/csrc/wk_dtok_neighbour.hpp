// wk_dtok_neighbour.hpp — does a line start a run?  Asked of the line before it alone (wk_dtok_fused.hpp).
//
// The line pass of the one-kernel tokenizer deals the lines of a window so that the line before a lane's line is always
// the lane below's, inside one wave: lanes 1..63 of a wave own 63 consecutive lines, and lane 0 is a *witness* -- it
// sums up the line in front of the wave's first own line once more (the last own line of the wave before, or of thread
// 511's wave in the trip before) and owns nothing: no probe, no word of `info[]` or `f_qn[]`, no bit in the ballots of
// run starts.  A trip of the workgroup's eight waves covers 8 x 63 = 504 lines (fw_line, fw_has below).  Only the
// window's first line has no line for its witness.  Each lane sums its line up in five words -- is there a line, is it
// mapped, the QNAME's length, and the QNAME's first 16 bytes (those behind its end cleared) -- and hands them one lane
// up; nothing goes through LDS and no lane waits for another wave.  fn_verdict says what the two summaries settle: a
// QNAME of at most 16 bytes is compared whole, a longer one can be told apart from the one before by its length or its
// first 16 bytes and is left to the kernel's byte compare where those agree.  A line whose neighbour is no mapped line
// (the window's first line, a line behind unmapped ones) is left to the kernel's search as well; a wave that holds such
// a line says so in one word of LDS, and a window in which no wave does skips the search pass and its barrier.  Plain
// functions, the same on the host and on the device: tests/test_dtok_neighbour_host.py holds the verdict against a byte
// compare of whole QNAMEs, tests/test_dtok_witness_host.py the dealing against plain enumeration.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WK_FN_FN __host__ __device__ __forceinline__
#else
#define WK_FN_FN inline
#endif

namespace wk {

constexpr uint32_t kFnLine = 1u << 16;     // there is a line (a lane without one hands 0 on)
constexpr uint32_t kFnMapped = 1u << 17;   // ... with a row of its own that names a subject
constexpr uint32_t kFnQn = 0xFFFFu;        // the QNAME's length (a window's offsets fit 16 bits)
constexpr uint32_t kFnBytes = 16;          // bytes of the QNAME that travel

struct FnLine {
    uint32_t meta;   // kFnLine | kFnMapped | length of the QNAME
    uint32_t b[4];   // its first min(length, 16) bytes, little-endian, zero behind them
};

enum FnVerdict : uint32_t { kFnStarts = 0, kFnContinues = 1, kFnUndecided = 2 };

// the low k bytes of w (k <= 8); no shift by 64
WK_FN_FN unsigned long long fn_low_bytes(unsigned long long w, uint32_t k) { return k >= 8u ? w : (w & ((1ull << (8u * k)) - 1ull)); }

// A line's summary from its first 16 bytes as two little-endian words (w0: bytes 0-7, w1: bytes 8-15; what lies
// behind the QNAME in them is cleared here) and its QNAME's length.
WK_FN_FN FnLine fn_line(bool mapped, uint32_t qn, unsigned long long w0, unsigned long long w1) {
    FnLine l;
    l.meta = kFnLine | (mapped ? kFnMapped : 0u) | (qn & kFnQn);
    const unsigned long long m0 = fn_low_bytes(w0, qn), m1 = qn > 8u ? fn_low_bytes(w1, qn - 8u) : 0ull;
    l.b[0] = (uint32_t)m0;
    l.b[1] = (uint32_t)(m0 >> 32);
    l.b[2] = (uint32_t)m1;
    l.b[3] = (uint32_t)(m1 >> 32);
    return l;
}
WK_FN_FN FnLine fn_no_line() { return FnLine{0u, {0u, 0u, 0u, 0u}}; }

// Mapped line `cur` behind line `prev`: does it start a run of equal QNAMEs?
WK_FN_FN FnVerdict fn_verdict(const FnLine& prev, const FnLine& cur) {
    if ((prev.meta & (kFnLine | kFnMapped)) != (kFnLine | kFnMapped)) return kFnUndecided;  // (the mapped line before is further back)
    const uint32_t diff = ((prev.meta ^ cur.meta) & kFnQn) | (prev.b[0] ^ cur.b[0]) | (prev.b[1] ^ cur.b[1]) | (prev.b[2] ^ cur.b[2]) | (prev.b[3] ^ cur.b[3]);
    if (diff) return kFnStarts;
    return (cur.meta & kFnQn) <= kFnBytes ? kFnContinues : kFnUndecided;
}

// ---- the dealing: 63 owners and a witness per wave ----
constexpr uint32_t kFwWave = 64;                      // lanes of a wave
constexpr uint32_t kFwWaves = 8;                      // waves of a workgroup
constexpr uint32_t kFwOwners = kFwWave - 1u;          // lines a wave owns per trip
constexpr uint32_t kFwTrip = kFwWaves * kFwOwners;    // lines a trip of the workgroup covers (504)

// The line of lane `lane` of wave `wave` in the trip that begins at line k0 (= first_line + 504 * trip): lanes 1..63
// own k0 + 63 * wave + lane - 1, lane 0 looks at the line in front of them.  (Unsigned: wave 0's witness of a window
// whose lines count from 0 gets 2^32 - 1, which fw_has turns down.)
WK_FN_FN uint32_t fw_line(uint32_t k0, uint32_t wave, uint32_t lane) { return k0 + kFwOwners * wave + lane - 1u; }
WK_FN_FN bool fw_witness(uint32_t lane) { return lane == 0u; }
// is k one of the window's whole lines [first_line, n_lines)?  (first_line is 0 or 1)
WK_FN_FN bool fw_has(uint32_t k, uint32_t first_line, uint32_t n_lines) { return k + 1u > first_line && k < n_lines; }
// (the line pass takes its trips as  for (k0 = first_line; k0 < n_lines; k0 += kFwTrip))

}  // namespace wk
