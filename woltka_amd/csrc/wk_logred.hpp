// wk_logred.hpp — the contribution log of size-normalised jobs (`--sizes`,
// wk_classify.hpp: log_append) reduced on the device: one row per distinct
// {feature, subject, job << 16 | divisor, group} with the number of times it
// occurs, appended to the row pile of wk_sized.hpp (sz_rows / sz_counts), so
// that the host folds every distinct row once and the log never leaves HBM.
//
// The log is immutable while it is reduced, and a row is *named by its index in
// the log*: a table slot holds the index of the first row that claimed it, and
// a probe that meets an occupied slot loads log[index] and compares all four
// words.  The key is therefore in memory before its index is published — one
// 32-bit CAS claims a slot, there is no half-written key, no 128-bit CAS, no
// lock, and no loop that waits for another lane's write.  Nothing relies on a
// hash being unique.
//
//   log_reduce_kernel   grid-stride over the rows, 16 B per lane.  A row first
//                       tries the workgroup's LDS front (a hot row — taxon logs
//                       are Zipf-skewed — then costs one device-scope atomic per
//                       workgroup, not per occurrence): kLogRedFrontSlots 64-bit
//                       words `index | check hash << 32`, claimed with one LDS
//                       CAS, home slot and the next one; a differing check hash
//                       skips the compare, an equal one is verified against
//                       log[index].  A row that finds no LDS slot goes to the
//                       global table: slots = a power of two >= 2 x rows,
//                       linear probing.  At the end the workgroup adds its LDS
//                       entries to the global table with their counts.  Slots
//                       never change once claimed and every lane probes in the
//                       same order, so a row cannot hold two global slots.
//   log_emit_kernel     one thread per global slot; a claimed slot appends
//                       log[index] and its count behind the rows of the pile
//                       (ballot + one returning atomic per wave, like
//                       sized_rows_kernel<true> and log_append).
#pragma once
#include "wk_device.hpp"

namespace wk {

constexpr uint32_t kLogRedEmpty = 0xFFFFFFFFu;   // no row index: the host refuses logs of 2^31 rows and more
constexpr uint32_t kLogRedThreads = 512;
// the LDS front: 4096 x (8 B word + 4 B count) = 48 KiB per workgroup.  Two
// 512-thread workgroups per CU (96 of the 160 KiB, 16 waves per CU): the flush
// of a hot row is then 2 x CUs atomics on one word (a few us), and a log of
// distinct rows loses little to a front that cannot help it.  (Chosen by that
// arithmetic; other sizes have not been measured.)
constexpr uint32_t kLogRedFrontSlots = 4096;
constexpr uint32_t kLogRedFrontBytes = kLogRedFrontSlots * 12u;
constexpr uint32_t kLogRedWgPerCu = 2;
constexpr uint32_t kLogRedEmitThreads = 256;

struct LogReduceArgs {
    const int4* log;               // rows [0, n_rows)
    uint32_t n_rows;               // < 2^31
    uint32_t* tidx;                // [slots] row index of the slot's row, or kLogRedEmpty
    uint32_t* tcnt;                // [slots] occurrences
    uint32_t mask;                 // slots - 1
    unsigned long long* n_distinct;  // += slots claimed
    int* err;
};

// one hash of all four words: the low bits pick the global slot, bits 20-31 the
// LDS slot, the high word is the check hash of the LDS front
__device__ __forceinline__ uint64_t log_row_hash(const int4& v) {
    const uint64_t a = (uint64_t)(uint32_t)v.x | ((uint64_t)(uint32_t)v.y << 32);
    const uint64_t b = (uint64_t)(uint32_t)v.z | ((uint64_t)(uint32_t)v.w << 32);
    return mix64(a ^ (mix64(b) * 0x9E3779B97F4A7C15ull));
}

__device__ __forceinline__ bool log_row_equal(const int4& a, const int4& b) {
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

// count `w` occurrences of row `v` = log[index]; true when this call claimed a slot
__device__ __forceinline__ bool log_table_add(const LogReduceArgs& a, uint32_t index, const int4& v, uint32_t home, uint32_t w) {
    uint32_t h = home & a.mask;
    for (uint64_t probe = 0; probe <= (uint64_t)a.mask; ++probe) {
        uint32_t cur = __hip_atomic_load(&a.tidx[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool claimed = false;
        if (cur == kLogRedEmpty) {
            cur = atomicCAS(&a.tidx[h], kLogRedEmpty, index);
            claimed = cur == kLogRedEmpty;
        }
        // (an index in the table is one a lane put there: below n_rows)
        if (claimed || (cur < a.n_rows && log_row_equal(a.log[cur], v))) {
            atomicAdd(&a.tcnt[h], w);
            return claimed;
        }
        h = (h + 1u) & a.mask;
    }
    atomicOr(a.err, kErrTableFull);  // (cannot happen: the table has two slots per row)
    return false;
}

__global__ void __launch_bounds__(kLogRedThreads) log_reduce_kernel(LogReduceArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* const fkey = reinterpret_cast<unsigned long long*>(smem);
    uint32_t* const fcnt = reinterpret_cast<uint32_t*>(smem + (size_t)kLogRedFrontSlots * 8);
    for (uint32_t i = threadIdx.x; i < kLogRedFrontSlots; i += kLogRedThreads) {
        fkey[i] = kEmptyKey;
        fcnt[i] = 0u;
    }
    __syncthreads();

    uint32_t claimed = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kLogRedThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kLogRedThreads + threadIdx.x; i < a.n_rows; i += stride) {
        const int4 v = a.log[i];
        const uint64_t h = log_row_hash(v);
        const unsigned long long mine = (unsigned long long)(uint32_t)i | (h & 0xFFFFFFFF00000000ull);
        uint32_t s = (uint32_t)(h >> 20) & (kLogRedFrontSlots - 1u);
        bool done = false;
#pragma unroll
        for (int probe = 0; probe < 2 && !done; ++probe) {
            // (the LDS address space spelled out, as in bucket_add: a ds_read, not a flat load)
            unsigned long long cur = *(const volatile __attribute__((address_space(3))) unsigned long long*)&fkey[s];
            bool mine_now = false;
            if (cur == kEmptyKey) {
                cur = atomicCAS(&fkey[s], (unsigned long long)kEmptyKey, mine);
                mine_now = cur == kEmptyKey;
            }
            if (!mine_now && (uint32_t)(cur >> 32) == (uint32_t)(h >> 32)) {
                const uint32_t at = (uint32_t)cur;
                mine_now = at < a.n_rows && log_row_equal(a.log[at], v);
            }
            if (mine_now) {
                atomicAdd(&fcnt[s], 1u);
                done = true;
            }
            s = (s + 1u) & (kLogRedFrontSlots - 1u);
        }
        if (!done) claimed += log_table_add(a, (uint32_t)i, v, (uint32_t)h, 1u) ? 1u : 0u;
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kLogRedFrontSlots; s += kLogRedThreads) {
        const unsigned long long cur = fkey[s];
        if (cur == kEmptyKey) continue;
        const uint32_t at = (uint32_t)cur;
        if (at >= a.n_rows) continue;  // (cannot happen)
        const int4 v = a.log[at];
        claimed += log_table_add(a, at, v, (uint32_t)log_row_hash(v), fcnt[s]) ? 1u : 0u;
    }
    // (kLogRedThreads is a whole number of waves and no lane has left: all 64 lanes sum)
    const unsigned long long n = wave_sum((unsigned long long)claimed);
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(a.n_distinct, n);
}

struct LogEmitArgs {
    const int4* log;
    uint32_t n_rows;
    const uint32_t* tidx;
    const uint32_t* tcnt;
    uint64_t slots;
    int4* out_rows;
    long long* out_counts;
    unsigned long long* cursor;    // rows appended by this launch
    unsigned long long base, cap;  // they go to [base, cap)
    int* err;
};

__global__ void __launch_bounds__(kLogRedEmitThreads) log_emit_kernel(LogEmitArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * kLogRedEmitThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t at_row = s < a.slots ? a.tidx[s] : kLogRedEmpty;
    const bool have = at_row < a.n_rows;
    const unsigned long long mask = __ballot(have);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned long long at = 0;
    if ((int)lane == leader) at = atomicAdd(a.cursor, (unsigned long long)__popcll(mask));
    at = __shfl(at, leader, kWave);
    if (!have) return;
    at += a.base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    if (at < a.cap) {
        a.out_rows[at] = a.log[at_row];
        a.out_counts[at] = (long long)a.tcnt[s];
    } else {
        atomicOr(a.err, kErrTableFull);  // (cannot happen: the pile was sized from the count)
    }
}

}  // namespace wk
