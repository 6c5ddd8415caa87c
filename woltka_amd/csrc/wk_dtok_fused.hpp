// wk_dtok_fused.hpp — the plain SAM tokenizer as ONE kernel.
//
// wk_dtok.hpp does a block of text in six launches (count -> tile_scan -> lines ->
// parse -> runs -> first_emit): the text is read three times and every kernel
// hands per-line arrays to the next through HBM (5.8x the text in fabric traffic,
// profiles/r05_e2e_lca_profile.json).  Here a workgroup keeps a window of text in
// LDS and does everything align.parse_sam_file + plain_mapper do to its lines
// (woltka/align.py:258-347, 47-115) in that one residency: line starts, the
// first three tabs, FLAG -> mate, RNAME -> dictionary, runs of equal QNAME, the
// subject *sets* of a run's reads, and the packed records (subject | position <<
// 23 | size << 27, wk_weigh.hpp).  Per-line arrays never leave LDS; the text is
// read from HBM once.
//
// Spans and ownership.  The text of a block is cut into one contiguous span per
// workgroup (FusedArgs::span bytes, the block in equal shares).  A run of equal
// QNAMEs belongs to the span its first mapped line starts in.  A workgroup
// walks its span window by window (at most kFzWin bytes in LDS at a time).  The
// first window looks kFzBack bytes back (the line before the span's first one:
// does that one continue a run?); a window owns the runs up to the last run
// start it sees -- that run may go on behind the window -- and the next window
// begins at that very line, which is known to start a run: nothing is looked at
// twice but the lines of that one run.  The last window looks kFzFwd bytes
// behind the span (the rest of its last run) and stops at the first run that
// starts at or behind the span's end; where it sees none, a span of several
// windows goes on from the start of its last run with wide windows: each
// reads up to kFzWin bytes from where it begins, past the kFzFwd bytes behind
// the span, until that run's end is seen.  A span of at most kFzTile bytes is
// one window -- kFzBack in front, the span, kFzFwd behind -- and looks no
// further.  A run that begins its window and does not end inside it -- a
// stretch of unmapped lines longer than a window behind or inside it -- is
// carried: the words of its mapped lines (at most kFzCarry) are put aside, the
// next window begins behind this one's last whole line with those words in
// front of its own lines' and compares its first mapped line's QNAME with the
// run's in global memory; the run's records leave where it ends.  A run of
// more mapped lines than that which does not end inside its window, a line
// that does not end inside the window it starts, more than kFzLines lines in
// a window, or a line before the span that cannot be found in the window's
// back part is nothing this kernel guesses about: the first three set
// kDtokSpill (the block is done again by the six kernels, which have no such
// limits), the last is looked up in global memory, as is the mapped line
// behind unmapped lines that fill a span's whole first window.
//
// Records.  Workgroups are persistent (a few per CU, one span each)
// and keep up to kFzCap records per slice of the subject table in LDS; a full
// buffer leaves with ONE returning atomic on the stream's cursor and coalesced
// stores.  (A reservation per tile and slice would be 12 k atomics on one cache
// line per 64 MB block: at ~11 ns each, serialised, 130 us -- more than the rest
// of the kernel.)  The histogram does not care about the order of the records.
//
// Anything the six kernels would leave to the host tokenizer (a line of fewer than
// four fields, a FLAG that is no number, both mate bits, a read of more than 16
// subjects) sets the same flags here; subjects the dictionary does not know are
// listed the same way.  The caller rolls the streams back and runs the unfused
// kernels on such a block.
#pragma once
#include "wk_dtok.hpp"
#include "wk_dtok_neighbour.hpp"
#include "wk_dtok_planes.hpp"
#include "wk_dtok_rounds.hpp"

namespace wk {

constexpr uint32_t kFzThreads = 512;
constexpr uint32_t kFzWaves = kFzThreads / kWave;
constexpr uint32_t kFzTile = 16384;
constexpr uint32_t kFzBack = 1024;
constexpr uint32_t kFzFwd = 3072;
constexpr uint32_t kFzWin = kFzTile + kFzBack + kFzFwd;
constexpr uint32_t kFzChunks = kFzWin / 16 + 1;   // (+1: the chunk behind the window's text, wk_dtok_rounds.hpp)
constexpr uint32_t kFzRounds = kFrMaxRounds;      // (the chunks are dealt to the waves in full rounds: wk_dtok_rounds.hpp)
static_assert(kFrChunks * 16u == kFzWin && kFrTailChunk + 1u == kFzChunks && kFrWaves == kFzWaves && kFrWave == kWave,
              "the dealing covers the window");
constexpr uint32_t kFzLines = 1024;   // lines of a window
constexpr uint32_t kFzStreams = 4;    // slices of the subject table (more: the unfused kernels)
constexpr uint32_t kFzCap = 1024;     // records kept per slice (>= kFzLines: a window's records always fit an empty buffer)
static_assert(kFzCap >= kFzLines, "a window's records fit an empty buffer");
static_assert(kFzWin + 32 < 65536, "window offsets fit 16 bits");
constexpr uint32_t kFzCarry = 256;    // mapped lines of a run that goes on behind its window, kept for the windows behind it
static_assert(kFzCarry + kFzLines <= kFpMaxLines && kFzThreads % kWave == 0, "a window's owned lines fit the planes, a wave's lines one word");

// Bits of FusedArgs::ablate that leave nothing out (the measuring instance gives the product's results with them):
// 1024 runs that instance as it is; kFzAblateTop has it load every window's text at the window's top, as the kernel
// did before it loaded a window ahead; kFzAblateTimeline has thread 0 of every kFzTlEvery-th workgroup store the wall
// clock (100 MHz) into FusedArgs::timeline, a row of kFzTlWords words per sampled workgroup: the kernel's entry, its
// exit, the windows it walked and its index, then kFzTlPer words for each of its first kFzTlWindows windows.
constexpr uint32_t kFzAblateTop = 2048, kFzAblateTimeline = 4096;
constexpr uint32_t kFzTlEvery = 64, kFzTlWindows = 24, kFzTlHead = 4, kFzTlPer = 12;
constexpr uint32_t kFzTlWords = kFzTlHead + kFzTlWindows * kFzTlPer;
enum : uint32_t {            // a window's words
    kFzTlBarrier = 0,        // behind the top barrier: the window before is through with the arrays
    kFzTlTop,                // the window's loads issued, where they were not a window before
    kFzTlText,               // the lane's chunks have arrived (behind a wait of this stamp's own)
    kFzTlStaged,             // behind the barrier that closes staging (text in LDS, newlines counted)
    kFzTlNumbered,           // behind the barrier that closes the lines' numbering
    kFzTlProbed,             // the line pass done: tabs, FLAG, RNAME, the dictionary's answers used
    kFzTlLines,              // behind the line pass's barrier
    kFzTlAhead,              // the ownership chain done and the next window's loads issued (where there are any)
    kFzTlPlanes,             // behind the planes' barrier
    kFzTlEnd,                // the records done: the window's end
    kFzTlInfo,               // no stamp: mode | the text was loaded a window ahead << 4 | a window follows << 5
};
static_assert(kFzTlInfo < kFzTlPer, "a window's words");

constexpr uint32_t kDtokSpill = 64;   // the fused kernel's limits (see above): the unfused kernels take the block

struct FusedArgs {
    const unsigned char* text;  // [n] + 64 readable bytes behind (zero)
    uint32_t n;
    uint32_t open_end;          // the text's last byte is no newline: a line ends at n
    uint32_t span;              // bytes per workgroup (a multiple of 16, >= 4096): the block in equal shares; the grid is ceil(n / span)
                                // (a multiple of 16: a span's first window begins at a chunk then and is at most kFzWin bytes, as the
                                // others are -- what wk_dtok_rounds.hpp's chunk behind the dealt ones rests on; the launch sites check it)
    const struct DictSlot8* dict8;
    const uint4* names16;       // by id
    uint32_t dict_mask;
    const unsigned char* arena;
    uint2* unknown;
    uint32_t unknown_cap;
    DtokState* state;
    DtokState* host_state;               // pinned host memory: the block's scalars, written by the last workgroup
    const unsigned long long* backup_prev;   // [kMaxStreams] the streams' cursors in front of this block (the begin kernel's, or the block before's backup_next)
    unsigned long long* backup_next;     // [kMaxStreams] the streams' cursors behind this block (= in front of the next)
    uint32_t* host_seq;                  // pinned host memory or null: `seq` is stored there (system scope, release) once host_state is written
    uint32_t seq;
    StreamSet streams;
    const int32_t* submap;      // tokenizer id -> subject index, when they differ (`--trim-sub`), or null
    uint32_t n_submap;
    uint32_t ablate;            // (measurement, wk_tune "fz_ablate": phases left out -- results are wrong then.  Read by
                                // dtok_fused_measure_kernel alone, which is launched when the word is not 0; bits 1 to 512 are
                                // tested, so 1024 runs that instance with nothing left out: tests/test_gpu_dtok_instances.py;
                                // 2048 and 4096: kFzAblateTop, kFzAblateTimeline)
    unsigned long long* timeline;   // (measurement) the stamps of kFzAblateTimeline, or null; the product's instance never reads it
};

// The block's reads (low half) and lines (high half) while the kernel runs: one word behind the DtokState, so that a
// workgroup leaves both with one add.  (A block's text is shorter than 2^32 bytes: neither half carries.)  The caller
// reserves sizeof(DtokState) + 64 bytes; whoever clears *state clears this word.
static_assert(sizeof(DtokState) % 8 == 0, "the packed totals are aligned");
__device__ __forceinline__ unsigned long long* fz_totals(DtokState* state) { return reinterpret_cast<unsigned long long*>(state + 1); }

// the streams' cursors put aside and the block's scalars cleared, in front of the fused kernel on its stream
__global__ void dtok_fused_begin_kernel(unsigned long long* __restrict__ backup, const unsigned long long* __restrict__ cursor, DtokState* state) {
    if (threadIdx.x < (uint32_t)kMaxStreams) backup[threadIdx.x] = cursor[threadIdx.x];
    if (threadIdx.x == 0) {
        *state = DtokState{0u, 0u, 0ull, 0ull, 0ull, 0u, 0u};
        *fz_totals(state) = 0ull;
    }
}

// Wave scans in registers (DPP: row shifts, then the two row broadcasts of gfx9) -- no trip through the LDS crossbar
// and no wait for it.  All 64 lanes must be active.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t fz_dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xF, false);
}
// inclusive sum over the lanes of a wave
__device__ __forceinline__ uint32_t fz_wave_scan(uint32_t v) {
    static_assert(kWave == 64, "four rows of sixteen lanes");
    v = fz_dpp_add<0x111, 0xF>(v);  // row_shr:1
    v = fz_dpp_add<0x112, 0xF>(v);  // row_shr:2
    v = fz_dpp_add<0x114, 0xF>(v);  // row_shr:4
    v = fz_dpp_add<0x118, 0xF>(v);  // row_shr:8
    v = fz_dpp_add<0x142, 0xA>(v);  // row_bcast:15 -- rows 1 and 3 take the row before's sum
    v = fz_dpp_add<0x143, 0xC>(v);  // row_bcast:31 -- rows 2 and 3 take the first half's sum
    return v;
}
__device__ __forceinline__ uint32_t fz_last_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1); }
__device__ __forceinline__ uint32_t fz_wave_sum(uint32_t v) { return fz_last_lane(fz_wave_scan(v)); }
__device__ __forceinline__ unsigned long long fz_first_lane64(unsigned long long v) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// (The newlines of a wave's chunks travel round by round as fields of one word: one scan numbers all three rounds and
// its last lane holds the wave's count -- fr_pack / fr_unpack, wk_dtok_rounds.hpp.)

// 16 aligned bytes of the text, read once: kept out of the way of what the L2 should hold (the dictionary)
__device__ __forceinline__ uint4 fz_load_stream(const unsigned char* p) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ unsigned long long fz_load64(const unsigned char* p) {
    unsigned long long w;
    __builtin_memcpy(&w, p, 8);  // (gfx950: one ds_read_b64 / global_load_dwordx2 whatever the alignment)
    return w;
}
__device__ __forceinline__ uint32_t fz_load32(const unsigned char* p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}
// 0x80 in every byte of w that equals c
__device__ __forceinline__ unsigned long long fz_eq_bytes(unsigned long long w, unsigned char c) {
    const unsigned long long x = w ^ (0x0101010101010101ull * c);
    return ~(((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x | 0x7F7F7F7F7F7F7F7Full);
}
__device__ __forceinline__ uint32_t fz_marks32(uint32_t w, uint32_t c4) {
    const uint32_t x = w ^ c4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// the low `k` bytes of w (k <= 8)
__device__ __forceinline__ unsigned long long fz_low_bytes(unsigned long long w, uint32_t k) {
    return k >= 8u ? w : (w & ((1ull << (8u * k)) - 1ull));
}

// wkh::hash_bytes (dtok_hash), eight bytes per load; `p` may be read up to 7 bytes past the name
__device__ __forceinline__ unsigned long long fz_hash(const unsigned char* p, uint32_t n) {
    unsigned long long h = 0xcbf29ce484222325ull ^ ((unsigned long long)n * 0x9E3779B97F4A7C15ull);
    while (n >= 8u) {
        h = (h ^ fz_load64(p)) * 0x100000001b3ull;
        h ^= h >> 29;
        p += 8;
        n -= 8u;
    }
    const unsigned long long v = n ? fz_low_bytes(fz_load64(p), n) : 0ull;
    h = (h ^ v) * 0x100000001b3ull;
    h ^= h >> 32;
    h *= 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// are the n bytes at x and y equal?  (both readable 7 bytes past their ends)
__device__ __forceinline__ bool fz_same(const unsigned char* x, const unsigned char* y, uint32_t n) {
    while (n >= 8u) {
        if (fz_load64(x) != fz_load64(y)) return false;
        x += 8;
        y += 8;
        n -= 8u;
    }
    return n == 0u || fz_low_bytes(fz_load64(x) ^ fz_load64(y), n) == 0ull;
}

// The dictionary as this kernel probes it: DictSlot8 + the names by id (wk_dtok.hpp).  (On config 3's text, 100 k
// subjects met evenly, the probe's time did not depend on the slots' size -- 16-byte slots + arena, 32-byte slots with
// the name inside, 8-byte slots + names by id all gave 27 us of a block's 125: it is two dependent trips to the L2 /
// the fabric either way.  The compact form is kept for text whose lines name few subjects, see there.)
// The subject name[0, rn) (in LDS) in the dictionary: its id, or kLineUnknown and the name listed for the host.  In
// two halves, so that the first slot's trip to memory is under way while the caller does something else.
struct FzProbe {
    unsigned long long hv, n0, n1;
    uint32_t h;
    uint2 slot;
};
__device__ __forceinline__ FzProbe fz_probe_begin(const FusedArgs& a, const unsigned char* name, uint32_t rn) {
    FzProbe p;
    p.n0 = p.n1 = 0ull;
    if (rn <= 15u) {
        // (the name's bytes read once, for the hash -- fz_hash(name, rn), written out for at most two words -- and for
        // the compare with names16; the second word lies inside txt's pad at the latest)
        const unsigned long long lo = fz_low_bytes(fz_load64(name), rn), hi = rn > 8u ? fz_low_bytes(fz_load64(name + 8), rn - 8u) : 0ull;
        p.n0 = lo;
        p.n1 = hi | ((unsigned long long)rn << 56);
        unsigned long long h = 0xcbf29ce484222325ull ^ ((unsigned long long)rn * 0x9E3779B97F4A7C15ull), v = lo;
        if (rn >= 8u) {
            h = (h ^ lo) * 0x100000001b3ull;
            h ^= h >> 29;
            v = hi;
        }
        h = (h ^ v) * 0x100000001b3ull;
        h ^= h >> 32;
        h *= 0x9E3779B97F4A7C15ull;
        p.hv = h ^ (h >> 29);
    } else {
        p.hv = fz_hash(name, rn);
    }
    p.h = (uint32_t)p.hv & a.dict_mask;
    p.slot = reinterpret_cast<const uint2*>(a.dict8)[p.h];
    return p;
}
__device__ __forceinline__ int32_t fz_probe_end(const FusedArgs& a, FzProbe p, const unsigned char* name, uint32_t rn, uint32_t abs_off) {
    for (;;) {
        const int32_t id = (int32_t)p.slot.y;
        if (id < 0) break;
        if (p.slot.x == (uint32_t)(p.hv >> 32)) {
            const uint4 nm = a.names16[id];
            const unsigned long long s0 = ((unsigned long long)nm.y << 32) | nm.x, s1 = ((unsigned long long)nm.w << 32) | nm.z;
            if (rn <= 15u) {
                if (s0 == p.n0 && s1 == p.n1) return id;
            } else if ((nm.w >> 24) == 0xFFu) {
                const unsigned char* full = a.arena + nm.x;  // [len:4][bytes], 16 zero bytes behind the arena
                if (fz_load32(full) == rn && fz_same(name, full + 4, rn)) return id;
            }
        }
        p.h = (p.h + 1u) & a.dict_mask;
        p.slot = reinterpret_cast<const uint2*>(a.dict8)[p.h];
    }
    const uint32_t at = atomicAdd(&a.state->n_unknown, 1u);
    if (at < a.unknown_cap)
        a.unknown[at] = make_uint2(abs_off, rn);
    else
        atomicOr(&a.state->flags, kDtokUnknownFull);
    return kLineUnknown;
}

// The mapped line before text position `at` (a line start) that no window holds: its QNAME compared with
// the n bytes at `q`.  true = the line at `at` starts a run.  (Global memory, a byte at a time: a span whose
// kFzBack bytes in front hold no complete mapped line -- long or unmapped lines --, or a window behind one that
// held unmapped lines only.)
__device__ bool fz_starts_run_slow(const unsigned char* __restrict__ text, uint32_t at, const unsigned char* q, uint32_t qn) {
    uint32_t pos = at;
    while (pos > 0u) {
        const uint32_t e = pos - 1u;  // the newline that ends the line before
        uint32_t s = e;
        while (s > 0u && text[s - 1u] != '\n') --s;
        uint32_t tab[3], nt = 0;
        for (uint32_t p = s; p < e && nt < 3u; ++p)
            if (text[p] == '\t') tab[nt++] = p;
        if (nt == 3u && !(tab[2] - tab[1] == 2u && text[tab[1] + 1u] == '*')) {
            if (tab[0] - s != qn) return true;
            for (uint32_t k = 0; k < qn; ++k)
                if (text[s + k] != q[k]) return true;
            return false;
        }
        pos = s;  // (unmapped, or no row at all -- its span sends the block to the host): the line before
    }
    return true;
}

// per-line word in LDS
constexpr uint32_t kFiSubj = (1u << 23) - 1u;   // subject index (all ones: not in the dictionary)
constexpr uint32_t kFiMateShift = 24;
constexpr uint32_t kFiMapped = 1u << 26;
constexpr uint32_t kFiStart = 1u << 27;          // starts a run of equal QNAMEs
constexpr uint32_t kFiUndecided = 1u << 28;      // (between the line pass and the search behind it) the lane below could not say whether the line starts a run
constexpr uint32_t kFiExcl = 1u << 29;           // names a subject of the exclusion set
constexpr uint32_t kFiDropped = 1u << 30;        // (on the line that starts a run) a line of the run does: the run is dropped whole
constexpr uint32_t kFiRead = kFiMapped | (3u << kFiMateShift);          // same read of a run: same mate (and mapped)
constexpr uint32_t kFiKey = kFiRead | kFiSubj;                          // ... and the same subject
constexpr uint32_t kFzPad = 8;                   // words in front of the lines' words (the duplicate walk reads eight at a time; nothing walks ahead any more)
static_assert(kFwWave == kWave && kFwWaves == kFzWaves, "the line pass's dealing is this workgroup's");

// The 0x80 marks of two words (bits 7, 15, 23, 31 of each) as bits 0-7, the first word's in the low nibble: the second
// word's marks go between the first one's (bits 4, 12, 20, 28), and one multiplication gathers all eight.  (Mark 8j [+4]
// times 2^(21 - 7j') lands on bit 8j - 7j' + 21 [+4]: 32 products on 32 different bits, so nothing carries, and only
// j = j' falls into bits 21-28.)
__device__ __forceinline__ uint32_t fz_octet(uint32_t z_lo, uint32_t z_hi) { return (((z_lo >> 7) | (z_hi >> 3)) * 0x00204081u >> 21) & 255u; }

// the newlines of a 16-byte chunk as bits 0-15
__device__ __forceinline__ uint32_t fz_newlines16(uint4 v) {
    return fz_octet(fz_marks32(v.x, 0x0A0A0A0Au), fz_marks32(v.y, 0x0A0A0A0Au)) | (fz_octet(fz_marks32(v.z, 0x0A0A0A0Au), fz_marks32(v.w, 0x0A0A0A0Au)) << 8);
}

// the tabs among the 32 bytes at p (LDS, any alignment) as the bits of one word
// (`q0`, `q1`, where given: the first 16 of those bytes, for the neighbour's compare -- wk_dtok_neighbour.hpp)
__device__ __forceinline__ uint32_t fz_tabs32(const unsigned char* p, unsigned long long* q0 = nullptr, unsigned long long* q1 = nullptr) {
    unsigned long long w[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) w[i] = fz_load64(p + 8u * i);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        m |= fz_octet(fz_marks32((uint32_t)w[i], 0x09090909u), fz_marks32((uint32_t)(w[i] >> 32), 0x09090909u)) << (8u * i);
    if (q0) {
        *q0 = w[0];
        *q1 = w[1];
    }
    return m;
}

// The kernel's body.  kMeasure = false is the product's kernel: FusedArgs::ablate is not read and every test of it
// folds away; kMeasure = true is the measuring instance of tools/fused_ablate.py, with the phases `ablate` names left
// out at run time (results are wrong then).  Both are instances of this one text: what is measured is what runs.
// kAhead: the text of the window that follows is asked for as soon as that window is known -- behind the ownership
// chain, in front of the planes and the records, which never look at txt[] -- into the registers the staging of the
// next trip reads; only a span's first window loads at its own top.  The measuring instance decides it at run time:
// bit 2048 of `ablate` = loads at every window's top, as before (like 1024, the bit leaves nothing out).
template <bool kMeasure, bool kAhead>
__device__ __forceinline__ void dtok_fused_body(const FusedArgs& a) {
    __shared__ __attribute__((aligned(16))) unsigned char txt[kFzChunks * 16 + 32];
    __shared__ uint16_t ls[kFzLines + 2];                                    // line starts (window offsets); ls[k + 1] - 1 = the newline of line k
    __shared__ uint16_t f_qn[kFzLines];                                      // QNAME length (the lines the lane below does not settle, and a run put aside)
    __shared__ __attribute__((aligned(16))) uint32_t info_[kFzPad + kFzCarry + kFzLines + kFzPad + 8];
    __shared__ uint32_t carry[kFzCarry];                                     // the words of a run's lines seen in windows before this one
    __shared__ unsigned long long planes[kFpPlanes][kFpWords];               // the owned lines as bits: run starts, first lines per mate (wk_dtok_planes.hpp)
    __shared__ uint32_t rbuf[kFzStreams][kFzCap];
    __shared__ unsigned long long fill_packed;   // records in the slices' buffers: 16 bits each (at most kFzCap and a trip's kFzThreads)
    static_assert(kFzStreams <= 4 && kFzCap + kFzThreads < 65536, "four 16-bit counts");
    __shared__ unsigned long long gbase[kFzStreams];
    __shared__ uint32_t wtot[kFzWaves];
    __shared__ unsigned long long gbase_out[kMaxStreams];                    // (the last workgroup) the streams' advance over the block
    __shared__ unsigned long long wg_totals;                                 // reads | lines << 32 of this workgroup (the exit)
    __shared__ uint32_t own[5];                                              // first run start in the span, first at or behind its end, last of the window; the lines put aside;
                                                                             // [4]: a wave holds a line its lane below did not settle (the search pass is needed)
    __shared__ uint32_t wg_flags;
    uint32_t* const info = info_ + kFzPad + kFzCarry;  // (lines of the window from 0 up, the carried lines of its first run below 0)

    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t wave_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);  // (in a scalar register: what depends on it alone is wave-uniform)
    const uint32_t n_streams = a.streams.n_streams;
    const uint32_t ablate = kMeasure ? a.ablate : 0u;
    const bool ahead = kMeasure ? !(ablate & kFzAblateTop) : kAhead;
    // (measurement) this workgroup's row of the timeline, where it is a sampled one; thread 0 stamps
    unsigned long long* tl = nullptr;
    if (kMeasure && (ablate & kFzAblateTimeline) && a.timeline != nullptr && blockIdx.x % kFzTlEvery == 0u)
        tl = a.timeline + (size_t)(blockIdx.x / kFzTlEvery) * kFzTlWords;
    auto stamp = [&](uint32_t word) {
        if (kMeasure && tl != nullptr && tid == 0) tl[word] = wall_clock64();
    };
    auto stamp_window = [&](uint32_t trip_, uint32_t which) {
        if (kMeasure && trip_ < kFzTlWindows) stamp(kFzTlHead + trip_ * kFzTlPer + which);
    };
    stamp(0);
    if (kMeasure && tl != nullptr && tid == 0) tl[3] = blockIdx.x;
    const int32_t* const submap = a.submap;
    // (the buffers' fill: the word in LDS is added to by the records loop alone; `fill` is what every thread read there
    // behind that loop's barrier, the same in all of them)
    unsigned long long fill = 0ull;
    if (tid == 0) fill_packed = 0ull;
    if (tid < 4u) reinterpret_cast<uint32_t*>(txt + kFrTailChunk * 16u)[tid] = 0u;  // (no wave's chunk and never text: wk_dtok_rounds.hpp)
    if (tid == 0) wg_flags = 0u;
    if (tid == 0) wg_totals = 0ull;
    uint32_t my_flags = 0, my_reads = 0, my_lines = 0;
    const uint32_t text_end = a.n + (a.open_end ? 1u : 0u);  // (a text without a last newline: as if one followed)

    // Every slice's buffer to its stream (every thread calls this): the slices' ranges are reserved side by side -- one
    // round trip to the cursors, whatever the number of slices -- and records that find no room raise kDtokSpill in
    // wg_flags, seen by the reserving lane.  (The histogram does not care about the records' order: a slice that is
    // not full leaves with the one that is.)  `have`: the buffers' fill, packed as fill_packed is.
    auto flush_all = [&](unsigned long long have, bool last) {
        __syncthreads();
        if (wave_s == 0u) {  // (the first wave's lanes, one per slice: a scalar test, and the compare made here)
            uint32_t xl = lane;
            asm volatile("" : "+v"(xl));
            if (xl < n_streams) {
                const uint32_t cnt = (ablate & 64u) ? 0u : (uint32_t)(have >> (16u * xl)) & 0xFFFFu;
                unsigned long long base = 0ull;
                if (cnt) {
                    base = atomicAdd(&a.streams.cursor[xl], (unsigned long long)cnt);
                    if (base + cnt > a.streams.cap) atomicOr(&wg_flags, kDtokSpill);
                }
                gbase[xl] = base;
            }
        }
        __syncthreads();
        for (uint32_t k = 0; k < n_streams; ++k) {
            const uint32_t cnt = (ablate & 64u) ? 0u : (uint32_t)(have >> (16u * k)) & 0xFFFFu;
            const unsigned long long base = gbase[k];
            for (uint32_t i = tid; i < cnt; i += kFzThreads)
                if (base + i < a.streams.cap) a.streams.out[k][base + i] = rbuf[k][i];
        }
        if (last) return;
        __syncthreads();  // (the buffers are the caller's again)
    };

    // The span [t0, t1) of this workgroup, window by window.  (Everything that steers the loop is the same in every
    // thread: the arguments, and words of LDS read behind a barrier.)
    const uint32_t t0 = blockIdx.x * a.span;   // (< n: the grid is ceil(n / span))
    const uint32_t t1 = a.n - t0 > a.span ? t0 + a.span : a.n;
    const uint32_t span_w1 = fr_min_end(t1, kFzFwd, text_end);  // (min(t1 + kFzFwd, text_end) without the 64-bit sum: wk_dtok_rounds.hpp)
    uint32_t wpos = t0 >= kFzBack ? t0 - kFzBack : 0u;  // the window's first byte of text
    uint32_t mode = 0u;       // 0: the span's first window; 1: the line at wpos starts a run; 2: it is not known whether it does
    uint32_t counted = t0;    // the newlines in front of this position are in my_lines (windows of a span overlap)
    bool wide = false;        // the span's last run did not end kFzFwd bytes behind the span: whole windows from its start on
    uint32_t nc = 0u;         // lines in `carry`: the mapped lines so far of a run that began in a window before and has not ended
    uint32_t cq_pos = 0u, cq_len = 0u;  // ... and where its QNAME is in the text
    const uint32_t max_trips = a.span / 16u + 2u;
    // the end of the text a window looks at, from its first chunk w0_ (one expression for the window's top and for the
    // loads issued a window ahead: both see the same [w0, w1))
    auto window_end = [&](uint32_t w0_, uint32_t mode_, bool wide_) {
        return fr_min_end(mode_ == 0u ? t0 : w0_, mode_ == 0u ? kFzTile + kFzFwd : kFzWin, wide_ ? text_end : span_w1);
    };
    // the chunks of this lane for the window [w0_, w1_): all loads under way before the first is looked at; a chunk
    // behind the window or the text is zeros
    auto load_window = [&](uint4 (&v_)[kFzRounds], uint32_t w0_, uint32_t w1_, uint32_t c0_, uint32_t rounds_) {
#pragma unroll
        for (uint32_t r = 0; r < kFzRounds; ++r) {
            const uint32_t p = w0_ + (c0_ + r * kWave + lane) * 16u;
            v_[r] = make_uint4(0u, 0u, 0u, 0u);
            if (r < rounds_ && p < a.n && p < w1_) v_[r] = fz_load_stream(a.text + p);  // (may pass n: the text's pad)
        }
    };
    uint4 v[kFzRounds];   // the lane's chunks of a window: asked for a window ahead (kAhead) or at the window's top
    bool loaded = false;  // ... they are under way: the window before asked for them
    for (uint32_t trip = 0;; ++trip) {
        // (never: every window begins at least one whole line behind the one before, or hands a carried run's records
        // over first -- wide windows too, which may follow one another; only a span's first wide look may begin where
        // the window before did)
        if (trip >= max_trips) {
            my_flags |= kDtokSpill;
            break;
        }
        const uint32_t w0 = wpos & ~15u;
        const uint32_t lead = wpos - w0;  // bytes of the line before in the first chunk (the first window begins at a chunk)
        // text positions [w0, w1) are looked at
        const uint32_t w1 = window_end(w0, mode, wide);
        const bool to_end = w1 == text_end;   // every line from here to the end of the text is whole
        const bool last_win = wide || w1 == span_w1;  // the span's last window: kFzFwd bytes behind the span, or the end of the text
        __syncthreads();  // (the window before is through with the arrays)
        stamp_window(trip, kFzTlBarrier);
        // The wave's index once more, as a scalar of this window's own (see the exit for the thread's): what is decided
        // by it below -- the first wave's stores, the rounds a wave runs, the waves in front of it -- is a scalar
        // compare made where it is used.  Compares with `wave_s` itself are the same in every window, and the compiler
        // makes each of them once, as a 64-bit mask of lanes in a pair of scalar registers the kernel does not have: a
        // lane of a VGPR written in front of the loop and two lane reads per use.
        uint32_t ws = wave_s;
        asm volatile("" : "+s"(ws));
        // (the first wave's lanes, found by a scalar test and compares with constants made here: the lane's number as
        // a value of its own, so that no mask and no word is kept through the window for these stores -- see the exit)
        if (ws == 0u) {
            uint32_t xl = lane;
            asm volatile("" : "+v"(xl));
            if (xl < 5u) own[xl] = xl < 2u ? 0xFFFFFFFFu : 0u;
            // (a walk back stops in front of the carried lines at the latest; it never gets there: their first one starts the run)
            if (xl < kFzPad) info[-(int32_t)nc - 1 - (int32_t)xl] = kFiStart;
        }
        for (uint32_t i = tid; i < nc; i += kFzThreads) info[(int32_t)i - (int32_t)nc] = carry[i];

        // ---- the window into LDS; newlines per 16-byte chunk ----
        // (a wave takes consecutive chunks, in full rounds -- wk_dtok_rounds.hpp: no barrier inside the scan below, and
        // the waves of two rounds skip the third, uniformly)
        // (wave_c0 goes into the lanes' addresses, which are kept; ws_c0 is the same number for the scalar tests)
        const uint32_t wave_c0 = fr_first_chunk(wave_s), ws_c0 = fr_first_chunk(ws), wave_rounds = fr_rounds(ws);
        // (a span's first window, and every window where nothing is loaded ahead; the others find their chunks under
        // way since the window before's ownership chain -- the registers are not written here then)
        const bool loaded_here = loaded;  // (measurement: for the timeline's info word)
        if (!loaded) load_window(v, w0, w1, wave_c0, wave_rounds);
        if (kMeasure && tl != nullptr) {  // (uniform)
            stamp_window(trip, kFzTlTop);
            __builtin_amdgcn_s_waitcnt(0x0F70);  // (vmcnt(0): the staging below would wait here for its first chunk anyway)
            stamp_window(trip, kFzTlText);
        }
        uint32_t marks[kFzRounds];
        uint32_t nl_packed = 0;
        bool blank = false;  // (a chunk of more newlines than are counted: an empty line, see fr_chunk_marks)
        // (the limits below in scalar registers: what a wave's 64 chunks of a round lie inside is decided once per wave)
        const uint32_t in_lo = max(wpos, counted), in_hi = min(min(w1, a.n), t1);
#pragma unroll
        for (uint32_t r = 0; r < kFzRounds; ++r) {
            const uint32_t c = wave_c0 + r * kWave + lane;
            const uint32_t p = w0 + c * 16u;
            marks[r] = 0u;
            if (r >= wave_rounds) continue;  // (wave-uniform)
            // The interior: all 64 chunks are text of this window from their first byte to their last, and their
            // newlines are this span's to count -- none of the corrections of the other branch applies.  (Almost
            // every round of almost every window; what touches the window's or the span's ends or the overlap with
            // the window before goes the other way.)
            const uint32_t rp0 = w0 + (ws_c0 + r * kWave) * 16u;  // (the wave's first chunk of the round)
            const bool interior = rp0 >= in_lo && fr_fits(rp0, kWave * 16u, in_hi);
            *reinterpret_cast<uint4*>(txt + c * 16u) = v[r];
            if (interior) {  // (wave-uniform, scalar compares)
                const uint32_t m = fr_chunk_marks(fz_newlines16(v[r]), &blank);
                const uint32_t cnt = (uint32_t)__popc(m);
                my_lines += cnt;
                marks[r] = m;
                nl_packed |= fr_pack(cnt, r);
            } else if (p < w1) {
                uint32_t m = fz_newlines16(v[r]);
                if (p + 16u > a.n) m &= p >= a.n ? 0u : (1u << (a.n - p)) - 1u;  // (nothing behind n is text)
                if (p >= counted && p < t1) my_lines += (uint32_t)__popc(m);     // (the block's lines: counted in the span they end in, once)
                if (a.n - p < 16u) m |= a.open_end << (a.n - p);  // (n in [p, p + 16) ends an open last line: open_end is 0 or 1)
                if (p + 16u > w1) m &= (1u << (w1 - p)) - 1u;
                if (p < wpos) m &= ~((1u << (wpos - p)) - 1u);                   // (the tail of the line before is no text of this window)
                m = fr_chunk_marks(m, &blank);
                marks[r] = m;
                nl_packed |= fr_pack((uint32_t)__popc(m), r);
            }
        }
        if (blank && !(ablate & 16u)) my_flags |= kDtokShortLine;  // (16: the measurement that leaves that flag out)
        // (one scan in registers: the wave's count now, the lines' numbers behind the barrier)
        const uint32_t nl_inc = fz_wave_scan(nl_packed);
        const uint32_t nl_wave = fz_last_lane(nl_inc);
        if (lane == 0) wtot[wave] = fr_total(nl_wave);
        __syncthreads();
        stamp_window(trip, kFzTlStaged);
        // (the waves' counts as scalars -- every lane reads the same words --, so that "the waves in front" is a scalar
        // compare with the wave's index and no mask of threads is kept through the window for it)
        uint32_t before = 0, total_nl = 0;
#pragma unroll
        for (uint32_t w = 0; w < kFzWaves; ++w) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)wtot[w]);
            before += w < ws ? t : 0u;
            total_nl += t;
        }
        // lines of the window: line k = [ls[k], ls[k + 1] - 1), k < total_nl whole (line 0 of a span's first window only
        // when it starts the text: that window begins in the middle of a line, the others at one)
        const bool too_many = total_nl + 1u > kFzLines || (ablate & (32u | 512u));
        if (too_many) {
            if (!(ablate & 512u)) my_flags |= kDtokSpill;
        } else {
            if (tid == 0) ls[0] = (uint16_t)lead;
            uint32_t line = before;  // newlines in front of this wave's chunks
#pragma unroll
            for (uint32_t r = 0; r < kFzRounds; ++r) {
                if (r >= wave_rounds) continue;  // (wave-uniform)
                const uint32_t c = wave_c0 + r * kWave + lane;
                uint32_t at = line + fr_unpack(nl_inc, r) - (uint32_t)__popc(marks[r]);
                uint32_t m = marks[r];
                while (m) {
                    const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
                    ls[++at] = (uint16_t)(c * 16u + b + 1u);
                    m &= m - 1u;
                }
                line += fr_unpack(nl_wave, r);
            }
        }
        __syncthreads();
        stamp_window(trip, kFzTlNumbered);
        // A line that STARTS in this span and does not end inside the span's last window is a line nobody sees whole:
        // its span is the one that would own a run it starts, and the spans behind it find no run start in it.  (Lines
        // of more than kFzFwd bytes -- SEQ / QUAL of a long read kept; text that comes through the column trim has
        // none.)  In a window that is not the last, the next window begins in front of that line -- or does not get
        // ahead, below.
        // the first byte behind the window's last newline
        const uint32_t trail = too_many ? wpos : w0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ls[total_nl]);
        if (!too_many && last_win && trail >= t0 && trail < t1) my_flags |= kDtokSpill;
        const uint32_t first_line = mode != 0u || w0 == 0u ? 0u : 1u;
        const uint32_t n_lines = too_many ? 0u : total_nl;  // whole lines: [first_line, n_lines)
        if (tid == 0 && first_line) info[0] = 0u;

        // ---- a thread per line: three tabs, FLAG, RNAME; its subject; does it start a run? ----
        // Lanes 1..63 of a wave own 63 consecutive lines and lane 0 is their witness (wk_dtok_neighbour.hpp): it sums up
        // the line in front of them once more and owns nothing, so the line before a lane's line is the lane below's in
        // every wave.  A mapped line at or behind t0 learns from that lane's summary whether it starts a run while the
        // dictionary slot of its subject is on its way.  What the neighbour does not settle -- it is unmapped, the QNAMEs
        // are longer than 16 bytes and agree that far, the window's first line where nothing says it starts a run -- is
        // marked kFiUndecided, the wave says so in own[4], and the search behind the barrier settles it.  (Every lane
        // takes every trip: the lanes exchange words.  The lines behind the last owned run are looked up for nothing:
        // the rest of one run, and once per span what the kFzFwd bytes behind it hold.)
        // (the line the window before stopped at, or the first of the text: it starts a run, no search needed)
        const bool first_starts = nc == 0u && (mode == 1u || wpos == 0u);
        for (uint32_t k0 = first_line; k0 < n_lines; k0 += kFwTrip) {
            const uint32_t k = fw_line(k0, wave, lane);
            const bool has = fw_has(k, first_line, n_lines), owner = !fw_witness(lane);
            uint32_t word = 0, s = 0, qn = 0, rb = 0, rn = 0;
            unsigned long long q0 = 0ull, q1 = 0ull;
            if (has) {
                s = ls[k];
                const uint32_t e = (uint32_t)ls[k + 1] - 1u;
                // The tabs of the line's first 32 bytes as one mask, the bits at or behind the line's end cleared (a short
                // line's 32 bytes reach into the next line), and its three lowest bits taken: no loop, no indexed array.
                // (The 32 bytes lie inside txt wherever the line starts: 32 bytes of pad behind the last chunk.)
                uint32_t tab[3] = {0, 0, 0}, nt = 0;
                if (!(ablate & 256u)) {
                    uint32_t m = fz_tabs32(txt + s, &q0, &q1);
                    if (e - s < 32u) m &= (1u << (e - s)) - 1u;
                    nt = min((uint32_t)__popc(m), 3u);
                    tab[0] = s + (uint32_t)__ffs((int)m) - 1u;
                    m &= m - 1u;
                    tab[1] = s + (uint32_t)__ffs((int)m) - 1u;
                    m &= m - 1u;
                    tab[2] = s + (uint32_t)__ffs((int)m) - 1u;  // (the first `nt` of the three are tabs; the others are not looked at)
                    // fewer than three and the line goes on: a QNAME or an RNAME of some length (rare on the texts measured)
                    for (uint32_t p = s + 32u; nt < 3u && p < e; p += 32u) {
                        m = fz_tabs32(txt + p);
                        if (e - p < 32u) m &= (1u << (e - p)) - 1u;
                        for (; m && nt < 3u; m &= m - 1u) {
                            const uint32_t q = p + (uint32_t)__ffs((int)m) - 1u;
                            if (nt == 0u)
                                tab[0] = q;
                            else if (nt == 1u)
                                tab[1] = q;
                            else
                                tab[2] = q;
                            ++nt;
                        }
                    }
                }
                if (ablate & 16u) {
                } else if (nt < 3u) {  // not `qname, flag, rname, _ = line.split('\t', 3)` (align.py:313)
                    my_flags |= kDtokShortLine;
                } else {
                    const uint32_t fl = tab[1] - tab[0] - 1u;
                    const unsigned long long fw = fz_load64(txt + tab[0] + 1u);
                    uint32_t flag = 0;
                    bool digits = fl >= 1u && fl <= 6u;
                    for (uint32_t i = 0; i < fl && i < 6u; ++i) {
                        const uint32_t d = ((uint32_t)(fw >> (8u * i)) & 0xFFu) - (uint32_t)'0';
                        digits &= d <= 9u;
                        flag = flag * 10u + d;
                    }
                    rb = tab[1] + 1u;
                    rn = tab[2] - rb;
                    if (!digits) {
                        my_flags |= kDtokShortLine;
                    } else if (rn == 1u && txt[rb] == '*') {
                        // unmapped: skipped before anything else (align.py:318-319)
                    } else {
                        const uint32_t mate = (flag >> 6) & 3u;
                        if (mate == 3u) my_flags |= kDtokBothMates;
                        word = kFiMapped | (mate << kFiMateShift);
                        qn = tab[0] - s;
                        if (owner) f_qn[k] = (uint16_t)qn;
                    }
                }
            }
            // (every lane again)  The subject of a mapped line at or behind t0 (only a first window has lines in front
            // of it): the first slot is asked for here and looked at behind the exchange.
            const bool mapped = (word & kFiMapped) != 0u, look = owner && mapped && w0 + s >= t0;
            const unsigned char* const name = txt + rb;
            FzProbe probe;
            if (look && !(ablate & 1u)) probe = fz_probe_begin(a, name, rn);
            // the line's summary one lane up; the witness takes "no line" and has no use for it
            const FnLine me = has ? fn_line(mapped, qn, q0, q1) : fn_no_line();
            FnLine prev;
            prev.meta = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)me.meta, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) prev.b[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)me.b[i], 0x138, 0xF, 0xF, false);
            const uint32_t verdict = ((ablate & 8u) || (first_starts && k == first_line)) ? (uint32_t)kFnStarts : (uint32_t)fn_verdict(prev, me);
            const bool start = look && verdict == kFnStarts;
            const unsigned long long b_und = __ballot(look && verdict == kFnUndecided);  // (every lane votes: not behind `lane == 0 &&`)
            if (lane == 0 && b_und != 0ull) own[4] = 1u;  // (every such wave stores the same word)
            if (look) {
                int32_t sid = (ablate & 1u) ? (int32_t)(fz_load32(name + 4) % 1000u) : fz_probe_end(a, probe, name, rn, w0 + rb);
                bool excluded = false;
                if (submap && sid >= 0) {
                    if ((uint32_t)sid < a.n_submap) {
                        sid = submap[sid];
                        if (sid == kLineExcluded) {  // (`--exclude`: the run goes, all its mates; align.py:47-115)
                            excluded = true;
                            sid = 0;
                        }
                    } else {  // (a name the host has not mapped yet: the block is done again)
                        my_flags |= kDtokSpill;
                        sid = -1;
                    }
                }
                word |= (start ? kFiStart : 0u) | (verdict == kFnUndecided ? kFiUndecided : 0u) | (excluded ? kFiExcl : 0u) |
                        (sid < 0 ? kFiSubj : ((uint32_t)sid & kFiSubj));
            }
            if (has && owner) info[k] = word;  // (the line's whole word, once)
            // The window's run starts: k rises with the lane (the witness's is one below lane 1's and raises no bit), so
            // a wave's first and last are its ballots' lowest and highest bits -- one lane tells own[].
            const unsigned long long b_all = __ballot(start), b_in = __ballot(start && w0 + s < t1), b_out = b_all & ~b_in;
            if (lane == 0 && b_all) {
                if (b_in) atomicMin(&own[0], k + (uint32_t)__builtin_ctzll(b_in));
                if (b_out) atomicMin(&own[1], k + (uint32_t)__builtin_ctzll(b_out));
                atomicMax(&own[2], k + 63u - (uint32_t)__builtin_clzll(b_all));
            }
        }
        stamp_window(trip, kFzTlProbed);
        __syncthreads();
        stamp_window(trip, kFzTlLines);
        // ---- what the lane below did not settle: the search back ----
        // (What every mapped line used to do: the mapped line before it searched for, the QNAMEs compared byte by byte.
        // own[4], read behind the barrier and the same in every thread, says whether any wave holds such a line: text
        // of short QNAMEs and few unmapped lines hardly ever comes here (a first window's lines in front of t0 are
        // neighbours like any other), and a window that does not skips this pass and the barrier that closes it.  The
        // starts of the line pass are in own[0..2] behind the barrier above.  Lines are dealt k0 + tid here: a line's
        // word is read from info[], whoever wrote it.)
        if (__builtin_amdgcn_readfirstlane((int)own[4])) {
        for (uint32_t k0 = first_line; k0 < n_lines; k0 += kFzThreads) {
            const uint32_t k = k0 + tid;
            const uint32_t mk = k < n_lines ? info[k] : 0u;
            const bool und = (mk & kFiUndecided) != 0u;
            bool start = false;
            if (__ballot(und) != 0ull) {  // (wave-uniform)
                if (und) {
                    uint32_t j = k;
                    bool found = false;
                    while (j > first_line) {
                        --j;
                        if (info[j] & kFiMapped) {
                            found = true;
                            break;
                        }
                    }
                    if (found)
                        start = f_qn[j] != f_qn[k] || !fz_same(txt + ls[k], txt + ls[j], f_qn[k]);
                    else if (nc)  // (the mapped line before is the carried run's last)
                        start = f_qn[k] != cq_len || !fz_same(txt + ls[k], a.text + cq_pos, cq_len);
                    else if (mode == 1u || wpos == 0u)  // (the line the window before stopped at, or the first of the text)
                        start = true;
                    else
                        start = fz_starts_run_slow(a.text, w0 + ls[first_line], txt + ls[k], f_qn[k]);
                }
            }
            if (mk & kFiUndecided) {
                // (this thread's own word; the others look at its mapped bit only)
                info[k] = (mk & ~kFiUndecided) | (start ? kFiStart : 0u);
                if (start) {
                    atomicMin(&own[w0 + ls[k] < t1 ? 0 : 1], k);
                    atomicMax(&own[2], k);
                }
            }
        }
        __syncthreads();
        }
        // Owned lines [ka, kb): from the first run that starts in the span (a first window), the window's first line or
        // the carried lines (below 0) to the first run that starts at or behind the span's end, or -- where the window
        // sees none -- to the last run start it sees: that run may go on behind the window, and the next window begins
        // with it.  A run that begins its window and does not end in it (a stretch of unmapped lines behind it, say) is
        // carried: its lines' words are put aside, the next window begins behind this one's last whole line and has
        // them in front of its own.  `more`: there is a next window, and it begins at `next`.
        const uint32_t o0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)own[0]), o1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)own[1]);
        const uint32_t last = (uint32_t)__builtin_amdgcn_readfirstlane((int)own[2]);  // (o0 != ~0: the window's last run start in the span)
        const uint32_t lpos = w0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ls[o0 != 0xFFFFFFFFu ? last : 0u]);  // ... and where it is
        const bool has_first = nc != 0u || o0 != 0xFFFFFFFFu;
        const int32_t first_own = nc ? -(int32_t)nc : (int32_t)o0;
        int32_t ka = 0, kb = 0;
        uint32_t next = 0u, next_mode = 0u, nc_next = 0u;
        bool more = false, again = false, put_aside = false;
        if (too_many) {
            if ((ablate & (32u | 512u)) && !last_win) {  // (measurement: the loads and the newlines of every window)
                next = w1;
                next_mode = 2u;
                more = true;
            }
        } else if (o1 != 0xFFFFFFFFu) {  // the span ends here
            kb = (int32_t)o1;
            ka = has_first ? first_own : kb;
        } else if (to_end) {
            kb = (int32_t)n_lines;
            ka = has_first ? first_own : kb;
        } else if (last_win && a.span <= kFzTile) {
            // the span's last run may go on behind the window: a span of one window looks kFzFwd bytes ahead and no further
            if (o0 != 0xFFFFFFFFu) my_flags |= kDtokSpill;
        } else if (o0 != 0xFFFFFFFFu && (nc != 0u || last != o0 || lpos > wpos)) {
            // the runs in front of the last start are whole; on from that start (behind the span's end: whole windows)
            kb = (int32_t)last;
            ka = first_own;
            next = lpos;
            next_mode = 1u;
            more = true;
            again = last_win;
        } else if (o0 != 0xFFFFFFFFu && last_win && !wide) {
            // the span's last run begins this window and does not end kFzFwd bytes behind the span: once more, a whole window
            next = wpos;
            next_mode = 1u;
            more = again = true;
        } else if (o0 != 0xFFFFFFFFu || nc != 0u) {
            // one run from the window's first line (or from windows before) to its end: put aside, on behind the last whole line
            put_aside = true;
        } else if (!last_win) {  // no run starts in this window (unmapped lines, lines of a run of the span before): on behind its last whole line
            next = trail;
            next_mode = 2u;
            more = trail > wpos && trail < t1;  // (what starts at or behind t1 is the next span's)
            if (trail <= wpos) my_flags |= kDtokSpill;  // a line that does not end inside the window it starts
        }
        if (put_aside) {  // (uniform)
            if (tid == 0) {
                uint32_t c = nc;
                for (uint32_t k = first_line; k < n_lines; ++k) {
                    const uint32_t w = info[k];
                    if (w & kFiMapped) {
                        if (c < kFzCarry) carry[c] = w & ~kFiDropped;
                        ++c;
                    }
                }
                own[3] = c;  // (a word of its own: the other waves may still be reading own[0..2] above)
            }
            __syncthreads();
            nc_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)own[3]);
            if (nc_next > kFzCarry || trail <= wpos) {  // a run of more lines than are kept, or a line that does not end inside its window
                my_flags |= kDtokSpill;
                nc_next = 0u;
            } else {
                if (nc == 0u) {
                    cq_pos = wpos;
                    cq_len = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)f_qn[0]);
                }
                next = trail;
                next_mode = 2u;
                more = true;
                again = last_win;
            }
        }
        // ---- the next window's text asked for (kAhead) ----
        // The window that follows is fixed here, and everything from here to its staging works on info[], planes[],
        // rbuf[] and the buffers' fill, never on txt[] or on `v`: its chunks travel under the duplicate walk, the
        // planes, the records and the next window's top.  The same chunks, limits and predicate as a load at that
        // top: `next` becomes wpos, `next_mode` (never 0) mode, `again` wide.
        // (vmcnt(0), said out loud: every load of the line pass has been used by now, but the compiler's bookkeeping
        // keeps some of their registers "under way" along paths that drop them, and where such a path meets this one
        // they count as younger than the loads below -- the planes' and the records' first writes to those registers
        // would wait for the text.  Nothing is under way here, so this wait costs nothing.)
        __builtin_amdgcn_s_waitcnt(0x0F70);
        loaded = ahead && more;
        if (loaded) {  // (uniform)
            const uint32_t w0n = next & ~15u;
            load_window(v, w0n, window_end(w0n, next_mode, again), wave_c0, wave_rounds);
        }
        stamp_window(trip, kFzTlAhead);
        // ---- first line of its read (run, mate) that names its subject (the plain parsers keep sets, align.py:309) ----
        // (walks read eight lines' words at a time: one trip to the LDS per eight lines instead of two per line.)  What
        // the lanes find leaves as the planes' words: a wave's 64 lines are one word of each plane, a ballot each -- so
        // every wave takes every trip with all its lanes, and a lane without a line of its own says no to all five.
        for (int32_t k0 = ka; k0 < kb; k0 += (int32_t)kFzThreads) {  // (uniform trip count: ballots inside)
            const int32_t k = k0 + (int32_t)tid;
            const uint32_t mk = k < kb ? info[k] : 0u;
            const bool mapped = (mk & kFiMapped) != 0u, excl = mapped && (mk & kFiExcl);
            if (excl) {  // the line its run starts with learns that the run is dropped (read behind the barrier)
                int32_t j = k;
                while (!(info[j] & kFiStart)) --j;
                atomicOr(&info[j], kFiDropped);
            }
            bool dup = false;
            if (mapped && !excl && !(mk & kFiStart) && !(ablate & 2u)) {
                bool done = false;
                for (int32_t j = k; !done; j -= 8) {
                    uint32_t w[8];
#pragma unroll
                    for (uint32_t i = 0; i < 8; ++i) w[i] = info[j - 1 - (int32_t)i];
#pragma unroll
                    for (uint32_t i = 0; i < 8; ++i) {
                        dup |= !done && ((w[i] ^ mk) & kFiKey) == 0u;
                        done |= (w[i] & kFiStart) != 0u;
                    }
                }
            }
            // (a line of both mate bits has sent the block back already; it counts among its like, as it did in the walks)
            const bool first = mapped && !excl && !dup;
            const uint32_t mate = (mk >> kFiMateShift) & 3u;
            const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(k0 - ka) / kWave + wave));  // (the planes' word of this wave's 64 lines)
            const bool put = lane == 0 && wi < kFpWords;
            const unsigned long long p_start = __ballot(mapped && (mk & kFiStart));
            if (put) planes[kFpStart][wi] = p_start;
#pragma unroll
            for (uint32_t m = 0; m < 4; ++m) {
                const unsigned long long p_first = __ballot(first && mate == m);
                if (put) planes[kFpFirst + m][wi] = p_first;
            }
        }
        __syncthreads();
        stamp_window(trip, kFzTlPlanes);
        // ---- records: position and size inside the read ----
        for (int32_t k0 = ka; k0 < kb; k0 += (int32_t)kFzThreads) {  // (uniform trip count: barriers inside)
            const int32_t k = k0 + (int32_t)tid;
            bool rec = false;
            uint32_t word = 0, sl = 0, at = 0;
            const uint32_t li = (uint32_t)(k - ka);  // (bit li % 64 = lane of word li / 64 of the planes)
            const uint32_t mk = k < kb ? info[k] : 0u;
            const unsigned long long* const mine = planes[kFpFirst + ((mk >> kFiMateShift) & 3u)];
            if (k < kb && ((mine[li / 64u] >> (li % 64u)) & 1ull) && !(ablate & 4u)) {
                uint32_t pos = 0, size = 1;
                bool dropped = (mk & kFiStart) && (mk & kFiDropped);
                if (!(ablate & (2u | 128u))) {
                    // (the head and the end of the run from the starts' plane, the first lines of this mate between them
                    // counted; the run's first line knows whether the run is dropped)
                    const FpRead r = fp_read(planes[kFpStart], mine, li, (uint32_t)(kb - ka));
                    pos = r.pos;
                    size = r.size;
                    dropped = (info[ka + (int32_t)r.head] & kFiDropped) != 0u;
                }
                if (size > (uint32_t)WK_WEIGHT_MAX_K) my_flags |= kDtokBigRead;
                const uint32_t s = mk & kFiSubj;
                if (s != kFiSubj && !dropped) {  // (kFiSubj: a subject the dictionary does not know -- the block is done again anyway)
                    rec = true;
                    word = s | ((pos & 15u) << kWordSubjBits) | ((size & 31u) << kWordSizeShift);
                    sl = s / kSliceBins;
                    if (sl >= n_streams) sl = n_streams - 1u;  // (a subject beyond the table: the histogram reports it)
                    my_reads += pos == 0u ? 1u : 0u;
                }
            }
            // A place in the slice's buffer: ONE LDS atomic per wave on the buffers' fill itself (the slices' counts are
            // 16-bit fields of one word), so what comes back are places in the buffers.
            {
                unsigned long long add = 0;
                uint32_t mine_before = 0;
                for (uint32_t s2 = 0; s2 < n_streams; ++s2) {
                    const unsigned long long m = __ballot(rec && sl == s2);
                    add |= (unsigned long long)__popcll(m) << (16u * s2);
                    if (rec && sl == s2) mine_before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                }
                if (add) {  // (wave-uniform)
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(&fill_packed, add);
                    base = fz_first_lane64(base);
                    at = (uint32_t)(base >> (16u * sl)) & 0xFFFFu;
                    at += mine_before;
                }
            }
            __syncthreads();
            // (every thread reads the same word: the fill with this trip's records.  A field above kFzCap -- 0x7BFF more
            // reaches bit 15, and no field carries: it is at most kFzCap + kFzThreads -- and the buffers leave first as
            // they were before the trip, `fill`; this trip's places move down by that much, and so does the word.)
            unsigned long long now = fz_first_lane64(fill_packed);
            static_assert(kFzCap + 0x7BFFu == 0x7FFFu && 2u * kFzCap + kFzThreads + 0x7BFFu < 0x10000u, "the full test");
            if ((now + 0x7BFF7BFF7BFF7BFFull) & 0x8000800080008000ull) {  // (uniform, and rare)
                flush_all(fill, false);
                at -= (uint32_t)(fill >> (16u * sl)) & 0xFFFFu;
                now -= fill;  // (field by field: none is below the fill's)
                if (tid == 0) fill_packed = now;
            }
            if (rec) rbuf[sl][at] = word;
            fill = now;
            // (Nobody adds to the word before everybody has read it: a window's first trip is behind the barriers of
            // the window's top, a trip that follows another behind this one.  The same barrier stands between thread
            // 0's store above and the next add.)
            if (k0 + (int32_t)kFzThreads < kb) __syncthreads();
        }
        stamp_window(trip, kFzTlEnd);
        if (kMeasure && tl != nullptr && tid == 0) {
            tl[2] = trip + 1u;
            if (trip < kFzTlWindows) tl[kFzTlHead + trip * kFzTlPer + kFzTlInfo] = mode | (loaded_here ? 16u : 0u) | (more ? 32u : 0u);
        }
        if (!more) break;
        wpos = next;
        mode = next_mode;
        wide = again;
        nc = nc_next;
        counted = w1;  // (a multiple of 16, or the end of the text: behind that no newline is counted)
    }
    // ---- the exit: two rounds of returning atomics per workgroup, the cursors and `done` ----
    // The workgroup's reads and lines as one word in LDS and its flags, behind flush_all's first barrier; the block's
    // records are the cursors' advance, which the last workgroup reads anyway.
    if (my_flags) atomicOr(&wg_flags, my_flags);
    {
        const uint32_t reads_w = fz_wave_sum(my_reads), lines_w = fz_wave_sum(my_lines);
        const unsigned long long t = ((unsigned long long)lines_w << 32) | reads_w;
        if (lane == 0 && t) atomicAdd(&wg_totals, t);
    }
    flush_all(fill, true);
    __syncthreads();
    if (tid == 0) {
        if (wg_totals) __hip_atomic_fetch_add(fz_totals(a.state), wg_totals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (nothing comes back)
        if (wg_flags) atomicOr(&a.state->flags, wg_flags);
        // The last workgroup through does what two more launches used to: the block's scalars to pinned host memory
        // (the host reads them once the stream has been waited for), the streams' cursors put aside as the next
        // block's "before", the scalars cleared for it.
        __threadfence();
        own[0] = atomicAdd(&a.state->done, 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (own[0]) {
        __threadfence();
        // (the cursors behind the block, and how far they are from those in front of it: the block's records)
        // (the thread's number once more, as a value of its own: addresses made of `tid` up there are not kept in
        // registers through the windows for this one use -- the kernel has none to spare)
        uint32_t xt = tid;
        asm volatile("" : "+v"(xt));
        if (xt < (uint32_t)kMaxStreams) {
            const unsigned long long cur = __hip_atomic_load(&a.streams.cursor[xt], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.backup_next[xt] = cur;
            gbase_out[xt] = xt < n_streams ? cur - a.backup_prev[xt] : 0ull;
        }
        __syncthreads();
        if (tid == 0) {
            DtokState st{};
            st.flags = __hip_atomic_load(&a.state->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st.n_unknown = __hip_atomic_load(&a.state->n_unknown, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long totals = __hip_atomic_load(fz_totals(a.state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (uint32_t k = 0; k < (uint32_t)kMaxStreams; ++k) st.n_out += gbase_out[k];
            st.n_reads = totals & 0xFFFFFFFFull;
            st.n_lines = totals >> 32;
            *a.host_state = st;
            *a.state = DtokState{0u, 0u, 0ull, 0ull, 0ull, 0u, 0u};
            *fz_totals(a.state) = 0ull;
            __threadfence_system();
            if (a.host_seq) __hip_atomic_store(a.host_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    stamp(1);
}

// the product's kernel
__global__ void __launch_bounds__(kFzThreads) __attribute__((amdgpu_waves_per_eu(6, 6))) dtok_fused_kernel(FusedArgs a) {
    dtok_fused_body<false, true>(a);
}
// the same with the measurement switches of wk_tune "fz_ablate" (launched exactly when that word is not 0)
__global__ void __launch_bounds__(kFzThreads) __attribute__((amdgpu_waves_per_eu(6, 6))) dtok_fused_measure_kernel(FusedArgs a) {
    dtok_fused_body<true, true>(a);
}

}  // namespace wk
