// wk_cover.hpp — subject coverage (`--outcov`) on the device: the union of the aligned ranges of every subject of
// one sample (range.merge_ranges / parse_ranges / calc_coverage, range.py:89-200).
//
// The pile: rows of (key: u64, end: i32), key = subject id << 32 | (uint32)(beg ^ 0x80000000) -- so the unsigned order
// of the keys is the (subject, signed beg) order -- in two buffers (the sort's ping-pong); the merged set of the
// sample so far sits in front of the rows appended since.  A compaction sorts the whole pile by key and merges it:
//
//   cover_append      the lines of an "ex" scan (wk_dtok.hpp: lsubj / lbeg / lend) or rows from the host -> the
//                     pile's tail.  Rank in the wave by ballot + popcount, one returning atomic per workgroup.
//   cover_hist        LSD radix sort, 8 bits a pass, only the digits that are not the same in every row (the append
//   cover_sum_tiles   keeps the OR and the AND of the keys): digit histogram of every chunk (a wave's 1024 contiguous
//   cover_scan_apply  rows) in LDS -> exclusive scan of the digit x chunk matrix -> stable scatter: a wave walks its
//   cover_scatter     chunk in row order, rows of equal digit ranked by ballots over the digit's bits.
//   cover_max_tiles   reach[i] = max end over rows <= i of the same subject: as the rows are sorted by subject, an
//   cover_max_scan    inclusive max-scan of subject << 32 | (uint32)(end ^ 0x80000000) -- a later subject always
//   cover_reach       dominates, nothing leaks across subjects, no segmented operator.  Three launches: per-tile
//                     maximum, scan of the tile maxima, apply + head flags + heads per tile.
//   cover_compact     a row is a head when its subject is new or beg > reach of the row before; a merged range is
//                     (beg[head], reach[last row before the next head]).
//
// Rows with end < beg (nothing the SAM and BLAST parsers produce; PAF columns may) are what merge_ranges makes of them:
// its sort is by (start, end), so with such rows in the pile the sort takes the digits of `end` first; and a head
// with end < beg stands alone (nothing starts at or before its end) and keeps its own end -- merge_ranges resets
// its running end at every head.
#pragma once
#include "wk_device.hpp"
#include "wk_ordinal.hpp"

namespace wk {

constexpr uint32_t kCoverThreads = 256;
constexpr uint32_t kCoverWaves = kCoverThreads / kWave;
constexpr uint32_t kCoverRounds = 16;                     // rows per lane of a sort chunk
constexpr uint32_t kCoverChunk = kWave * kCoverRounds;    // a wave's contiguous share of a pass: 1024 rows
constexpr uint32_t kCoverPer = 8;                         // rows (matrix entries) per thread of the scans
constexpr uint32_t kCoverTile = kCoverThreads * kCoverPer;  // 2048
constexpr uint32_t kCoverBias = 0x80000000u;
constexpr int64_t kCoverCapMin = 4096, kCoverCapMax = 1ll << 28, kCoverCapDefault = 1ll << 22;  // rows of a pile

struct CoverState {  // device scalars of the pile
    unsigned long long tail;     // rows in the current buffer, the merged set included
    unsigned long long key_or;   // over every row appended since the reset
    unsigned long long key_and;
    uint32_t end_or;             // of end ^ bias
    uint32_t end_and;
    uint32_t degenerate;         // some row with end < beg
    uint32_t overflow;           // a row found no room (the host reserves it: never set)
};

// rows [i0, i1) of (subj, beg, end) with subj >= 0 -> the pile's tail
__global__ void __launch_bounds__(kCoverThreads) cover_append_kernel(const int32_t* __restrict__ subj, const int32_t* __restrict__ beg,
                                                                     const int32_t* __restrict__ end, uint32_t i0, uint32_t i1,
                                                                     unsigned long long* __restrict__ keys, int32_t* __restrict__ ends,
                                                                     unsigned long long cap, CoverState* __restrict__ st) {
    __shared__ uint32_t w_cnt[kCoverWaves];
    __shared__ unsigned long long w_or[kCoverWaves], w_and[kCoverWaves];
    __shared__ uint32_t w_eor[kCoverWaves], w_eand[kCoverWaves], w_deg[kCoverWaves];
    __shared__ unsigned long long base;
    const uint32_t i = i0 + blockIdx.x * kCoverThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    bool keep = false;
    unsigned long long key = 0;
    int32_t e = 0, b = 0;
    if (i < i1) {
        const int32_t s = subj[i];
        if (s >= 0) {
            keep = true;
            b = beg[i];
            e = end[i];
            key = ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)((uint32_t)b ^ kCoverBias);
        }
    }
    const unsigned long long mask = __ballot(keep);
    const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    unsigned long long k_or = keep ? key : 0ull, k_and = keep ? key : ~0ull;
    uint32_t e_or = keep ? (uint32_t)e ^ kCoverBias : 0u, e_and = keep ? (uint32_t)e ^ kCoverBias : ~0u;
    uint32_t deg = keep && e < b ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        k_or |= __shfl_xor(k_or, off, kWave);
        k_and &= __shfl_xor(k_and, off, kWave);
        e_or |= __shfl_xor(e_or, off, kWave);
        e_and &= __shfl_xor(e_and, off, kWave);
        deg |= __shfl_xor(deg, off, kWave);
    }
    if (lane == 0) {
        w_cnt[wave] = (uint32_t)__popcll(mask);
        w_or[wave] = k_or;
        w_and[wave] = k_and;
        w_eor[wave] = e_or;
        w_eand[wave] = e_and;
        w_deg[wave] = deg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < kCoverWaves; ++w) {
            total += w_cnt[w];
            if (w) {
                w_or[0] |= w_or[w];
                w_and[0] &= w_and[w];
                w_eor[0] |= w_eor[w];
                w_eand[0] &= w_eand[w];
                w_deg[0] |= w_deg[w];
            }
        }
        if (total) {  // (one returning atomic per workgroup; the bits in use with it)
            base = atomicAdd(&st->tail, (unsigned long long)total);
            atomicOr(&st->key_or, w_or[0]);
            atomicAnd(&st->key_and, w_and[0]);
            atomicOr(&st->end_or, w_eor[0]);
            atomicAnd(&st->end_and, w_eand[0]);
            if (w_deg[0]) atomicOr(&st->degenerate, 1u);
        }
    }
    __syncthreads();
    if (!keep) return;
    unsigned long long at = base + rank;
    for (uint32_t w = 0; w < wave; ++w) at += w_cnt[w];
    if (at >= cap) {
        atomicOr(&st->overflow, 1u);
        return;
    }
    keys[at] = key;
    ends[at] = e;
}

// the tail as the host leaves it behind a compaction (the scan's total: the merged ranges)
__global__ void cover_set_tail_kernel(CoverState* st, const unsigned long long* total) { st->tail = *total; }

// ---- sort ---------------------------------------------------------------------------------------------------

struct CoverSortArgs {
    const unsigned long long* key_in;
    const int32_t* end_in;
    unsigned long long* key_out;
    int32_t* end_out;
    uint32_t n;
    uint32_t n_chunks;
    uint32_t shift;     // of the digit
    uint32_t from_end;  // the digit is one of end ^ bias (rows with end < beg in the pile: merge_ranges sorts by (start, end))
    uint32_t* hist;     // [256][n_chunks]: counts, then their exclusive prefix in (digit, chunk) order
    CoverState* st;     // (overflow: a row whose place is outside the pile -- histogram and scatter disagree; never set)
};

__device__ __forceinline__ uint32_t cover_digit(const CoverSortArgs& a, uint32_t row) {
    if (a.from_end) return (((uint32_t)a.end_in[row] ^ kCoverBias) >> a.shift) & 255u;
    return (uint32_t)(a.key_in[row] >> a.shift) & 255u;
}

__global__ void __launch_bounds__(kCoverThreads) cover_hist_kernel(CoverSortArgs a) {
    __shared__ uint32_t h[kCoverWaves][256];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t chunk = blockIdx.x * kCoverWaves + wave;
    for (uint32_t d = lane; d < 256u; d += kWave) h[wave][d] = 0u;
    __syncthreads();
    if (chunk < a.n_chunks) {
        const uint32_t first = chunk * kCoverChunk;
#pragma unroll 4
        for (uint32_t r = 0; r < kCoverRounds; ++r) {
            const uint32_t row = first + r * kWave + lane;
            if (row < a.n) atomicAdd(&h[wave][cover_digit(a, row)], 1u);
        }
    }
    __syncthreads();
    if (chunk < a.n_chunks)
        for (uint32_t d = lane; d < 256u; d += kWave) a.hist[(size_t)d * a.n_chunks + chunk] = h[wave][d];
}

// sums of the tiles of `kCoverTile` matrix entries (the scan of the sums: tile_scan_kernel, wk_ordinal.hpp)
__global__ void __launch_bounds__(kCoverThreads) cover_sum_tiles_kernel(const uint32_t* __restrict__ v, uint32_t n,
                                                                        unsigned long long* __restrict__ tile_sum) {
    __shared__ unsigned long long wsum[kCoverWaves];
    const uint32_t first = blockIdx.x * kCoverTile + threadIdx.x * kCoverPer;
    unsigned long long mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k)
        if (first + k < n) mine += v[first + k];
    mine = wave_sum(mine);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kCoverWaves; ++w) t += wsum[w];
        tile_sum[blockIdx.x] = t;
    }
}

// exclusive prefix of the thread's value over the workgroup (every thread calls)
__device__ __forceinline__ unsigned long long cover_block_prefix(unsigned long long mine, unsigned long long* wtot) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long inc = mine;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned long long up = __shfl_up(inc, off, kWave);
        if ((int)lane >= off) inc += up;
    }
    if (lane == kWave - 1) wtot[wave] = inc;
    __syncthreads();
    unsigned long long before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wtot[w];
    return before + inc - mine;
}

// v[i] -> the exclusive prefix over the whole matrix (below 2^32: the pile holds fewer rows)
__global__ void __launch_bounds__(kCoverThreads) cover_scan_apply_kernel(uint32_t* __restrict__ v, uint32_t n,
                                                                         const unsigned long long* __restrict__ tile_off) {
    __shared__ unsigned long long wtot[kCoverWaves];
    const uint32_t first = blockIdx.x * kCoverTile + threadIdx.x * kCoverPer;
    uint32_t x[kCoverPer];
    unsigned long long mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k) {
        x[k] = first + k < n ? v[first + k] : 0u;
        mine += x[k];
    }
    unsigned long long run = tile_off[blockIdx.x] + cover_block_prefix(mine, wtot);
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k) {
        if (first + k < n) v[first + k] = (uint32_t)run;
        run += x[k];
    }
}

// A wave moves its chunk in row order: rows of one digit keep their order (within the chunk by the rank among the
// lanes of equal digit and the rounds' running counts, across chunks by the matrix's order) -- LSD needs that.
__global__ void __launch_bounds__(kCoverThreads) cover_scatter_kernel(CoverSortArgs a) {
    __shared__ volatile uint32_t base[kCoverWaves][256];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t chunk = blockIdx.x * kCoverWaves + wave;
    if (chunk < a.n_chunks)
        for (uint32_t d = lane; d < 256u; d += kWave) base[wave][d] = a.hist[(size_t)d * a.n_chunks + chunk];
    __syncthreads();
    if (chunk >= a.n_chunks) return;
    const uint32_t first = chunk * kCoverChunk;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < kCoverRounds; ++r) {
        const uint32_t row = first + r * kWave + lane;
        const bool valid = row < a.n;
        unsigned long long key = 0;
        int32_t e = 0;
        uint32_t d = 0;
        if (valid) {
            key = a.key_in[row];
            e = a.end_in[row];
            d = a.from_end ? (((uint32_t)e ^ kCoverBias) >> a.shift) & 255u : (uint32_t)(key >> a.shift) & 255u;
        }
        unsigned long long same = __ballot(valid);   // the lanes of this lane's digit
#pragma unroll
        for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long m = __ballot(one);
            same &= one ? m : ~m;
        }
        uint32_t old = 0;
        if (valid) old = base[wave][d];
        __builtin_amdgcn_wave_barrier();   // (every lane has read its digit's count before a leader moves it on)
        if (valid && (same & below) == 0ull) base[wave][d] = old + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            const uint32_t at = old + (uint32_t)__popcll(same & below);
            if (at < a.n) {
                a.key_out[at] = key;
                a.end_out[at] = e;
            } else {
                atomicOr(&a.st->overflow, 1u);
            }
        }
    }
}

// ---- merge --------------------------------------------------------------------------------------------------

struct CoverMergeArgs {
    const unsigned long long* key;  // sorted; [n_tiles * kCoverTile] readable
    const int32_t* end;
    uint32_t n;
    int32_t* reach;                 // [n_tiles * kCoverTile]
    unsigned long long* tile_max;   // [n_tiles] maxima, then (cover_max_scan) the maximum over the tiles before
    unsigned long long* tile_heads; // [n_tiles]
    const unsigned long long* tile_off;  // heads in front of the tile
    unsigned long long* key_out;    // the merged rows
    int32_t* end_out;
};

__device__ __forceinline__ unsigned long long cover_reach_word(unsigned long long key, int32_t end) {
    return (key & 0xFFFFFFFF00000000ull) | (unsigned long long)((uint32_t)end ^ kCoverBias);
}
__device__ __forceinline__ int32_t cover_key_beg(unsigned long long key) { return (int32_t)((uint32_t)key ^ kCoverBias); }

// the thread's kCoverPer consecutive rows (the buffers are readable up to the tile's end)
__device__ __forceinline__ void cover_load_rows(const CoverMergeArgs& a, uint32_t first, unsigned long long (&key)[kCoverPer], int32_t (&end)[kCoverPer]) {
    const ulonglong2* kp = reinterpret_cast<const ulonglong2*>(a.key + first);
    const int4* ep = reinterpret_cast<const int4*>(a.end + first);
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer / 2; ++k) {
        const ulonglong2 t = kp[k];
        key[2 * k] = t.x;
        key[2 * k + 1] = t.y;
    }
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer / 4; ++k) {
        const int4 t = ep[k];
        end[4 * k] = t.x;
        end[4 * k + 1] = t.y;
        end[4 * k + 2] = t.z;
        end[4 * k + 3] = t.w;
    }
}

__device__ __forceinline__ unsigned long long cover_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(kCoverThreads) cover_max_tiles_kernel(CoverMergeArgs a) {
    __shared__ unsigned long long wmax[kCoverWaves];
    const uint32_t first = blockIdx.x * kCoverTile + threadIdx.x * kCoverPer;
    unsigned long long key[kCoverPer];
    int32_t end[kCoverPer];
    cover_load_rows(a, first, key, end);
    unsigned long long mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k)
        if (first + k < a.n) {
            const unsigned long long v = cover_reach_word(key[k], end[k]);
            mine = v > mine ? v : mine;
        }
    mine = cover_wave_max(mine);
    if ((threadIdx.x & (kWave - 1)) == 0) wmax[threadIdx.x / kWave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kCoverWaves; ++w) t = wmax[w] > t ? wmax[w] : t;
        a.tile_max[blockIdx.x] = t;
    }
}

// tile_max[t] -> the maximum over the tiles in front of t (one workgroup; the shape of tile_scan_kernel)
__global__ void __launch_bounds__(1024) cover_max_scan_kernel(unsigned long long* __restrict__ tile_max, uint32_t n_tiles) {
    __shared__ unsigned long long wave_tot[16];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, n_waves = blockDim.x / kWave;
    unsigned long long carry = 0;  // identical in every thread
    for (uint32_t base = 0; base < n_tiles; base += blockDim.x) {
        const uint32_t t = base + threadIdx.x;
        const unsigned long long v = t < n_tiles ? tile_max[t] : 0ull;
        unsigned long long inc = v;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const unsigned long long up = __shfl_up(inc, off, kWave);
            if ((int)lane >= off) inc = up > inc ? up : inc;
        }
        unsigned long long exc = __shfl_up(inc, 1, kWave);
        if (lane == 0) exc = 0ull;
        if (lane == kWave - 1) wave_tot[wave] = inc;
        __syncthreads();
        unsigned long long before = carry, round_max = carry;
        for (uint32_t q = 0; q < n_waves; ++q) {
            const unsigned long long w = wave_tot[q];
            if (q < wave) before = w > before ? w : before;
            round_max = w > round_max ? w : round_max;
        }
        if (t < n_tiles) tile_max[t] = exc > before ? exc : before;
        carry = round_max;
        __syncthreads();
    }
}

// is row i (> 0) a head, given the reach of the row before it?
__device__ __forceinline__ bool cover_is_head(unsigned long long key, unsigned long long key_before, int32_t reach_before) {
    return (key >> 32) != (key_before >> 32) || cover_key_beg(key) > reach_before;
}

// reach of every row (inclusive max-scan with the tiles' carry), heads per tile
__global__ void __launch_bounds__(kCoverThreads) cover_reach_kernel(CoverMergeArgs a) {
    __shared__ unsigned long long wmax[kCoverWaves];
    __shared__ unsigned long long wheads[kCoverWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t first = blockIdx.x * kCoverTile + threadIdx.x * kCoverPer;
    unsigned long long key[kCoverPer];
    int32_t end[kCoverPer];
    cover_load_rows(a, first, key, end);
    unsigned long long v[kCoverPer], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k) {
        v[k] = first + k < a.n ? cover_reach_word(key[k], end[k]) : 0ull;
        mine = v[k] > mine ? v[k] : mine;
    }
    unsigned long long inc = mine;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned long long up = __shfl_up(inc, off, kWave);
        if ((int)lane >= off) inc = up > inc ? up : inc;
    }
    unsigned long long exc = __shfl_up(inc, 1, kWave);
    if (lane == 0) exc = 0ull;
    if (lane == kWave - 1) wmax[wave] = inc;
    __syncthreads();
    unsigned long long run = a.tile_max[blockIdx.x];   // (the carry: cover_max_scan_kernel)
    for (uint32_t w = 0; w < wave; ++w) run = wmax[w] > run ? wmax[w] : run;
    run = exc > run ? exc : run;
    // `run`: the reach of the row before the thread's first (a word of an earlier subject, or 0, in front of a
    // subject's first row: its subject bits differ, or the row is row 0)
    uint32_t heads = 0;
    int32_t out[kCoverPer];
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k) {
        const uint32_t i = first + k;
        if (i < a.n) {
            const bool head = i == 0u || (key[k] >> 32) != (run >> 32) || cover_key_beg(key[k]) > (int32_t)((uint32_t)run ^ kCoverBias);
            heads += head ? 1u : 0u;
            run = v[k] > run ? v[k] : run;
        }
        out[k] = (int32_t)((uint32_t)run ^ kCoverBias);
    }
    int4* rp = reinterpret_cast<int4*>(a.reach + first);
    rp[0] = make_int4(out[0], out[1], out[2], out[3]);
    rp[1] = make_int4(out[4], out[5], out[6], out[7]);
    const unsigned long long hs = wave_sum((unsigned long long)heads);
    if (lane == 0) wheads[wave] = hs;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kCoverWaves; ++w) t += wheads[w];
        a.tile_heads[blockIdx.x] = t;
    }
}

// the merged rows: (subject, beg) of every head, the reach of the last row of its group
__global__ void __launch_bounds__(kCoverThreads) cover_compact_kernel(CoverMergeArgs a) {
    __shared__ unsigned long long wtot[kCoverWaves];
    const uint32_t first = blockIdx.x * kCoverTile + threadIdx.x * kCoverPer;
    unsigned long long key[kCoverPer];
    int32_t end[kCoverPer];
    cover_load_rows(a, first, key, end);
    int32_t reach[kCoverPer];
    {
        const int4* rp = reinterpret_cast<const int4*>(a.reach + first);
        const int4 r0 = rp[0], r1 = rp[1];
        reach[0] = r0.x, reach[1] = r0.y, reach[2] = r0.z, reach[3] = r0.w;
        reach[4] = r1.x, reach[5] = r1.y, reach[6] = r1.z, reach[7] = r1.w;
    }
    // head flags of the thread's rows and of the row behind them
    bool head[kCoverPer + 1];
    unsigned long long kb = 0;
    int32_t rb = 0;
    if (first > 0u && first < a.n) {
        kb = a.key[first - 1u];
        rb = a.reach[first - 1u];
    }
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k) {
        const uint32_t i = first + k;
        head[k] = i < a.n && (i == 0u || cover_is_head(key[k], kb, rb));
        mine += head[k] ? 1u : 0u;
        kb = key[k];
        rb = reach[k];
    }
    {
        const uint32_t i = first + kCoverPer;
        head[kCoverPer] = i >= a.n || cover_is_head(a.key[i], kb, rb);
    }
    unsigned long long at = a.tile_off[blockIdx.x] + cover_block_prefix((unsigned long long)mine, wtot);
#pragma unroll
    for (uint32_t k = 0; k < kCoverPer; ++k) {
        const uint32_t i = first + k;
        if (i >= a.n) break;
        if (head[k]) a.key_out[at++] = key[k];
        const bool last = i + 1u >= a.n || head[k + 1];
        // (`at` > 0 here: row 0 is a head.  A head with end < beg stands alone and keeps its end.)
        if (last) a.end_out[at - 1u] = head[k] && end[k] < cover_key_beg(key[k]) ? end[k] : reach[k];
    }
}

}  // namespace wk
