// wk_weigh_wide.hpp — the weighted histogram (wk_weigh.hpp) for subject tables of more slices than a team has
// workgroups: the "wide" layout, up to the packed word's 2^23 subjects (207 slices).
//
// The accumulation is one stream of packed words (more than kMaxStreams slices: nobody kept the records apart when
// they were appended).  The team layout reads that stream once per slice; beyond 32 slices a team no longer fits the
// device.  Here the records are partitioned by slice first, then every slice's records are histogrammed exactly once:
//
//   count    one pass over the words: an LDS histogram of bucket ids (bucket = slice of the subject table; an index
//            at or beyond the last bucket counts for the last one, where the histogram reports it) per workgroup,
//            added to bucket_count[] in HBM;
//   scan     one thread: exclusive scan of at most 207 counts -> where every bucket starts in the second buffer, and
//            the histogram's work list (wide_plan below: plain code, the same on the host, held against a plain
//            count by tests/test_weigh_wide_host.py);
//   scatter  per tile of kWideTile words: LDS counters give every word its rank inside its bucket's share of the
//            tile, one global atomic per non-empty bucket reserves that share's range, the tile is ordered by bucket
//            in LDS and stored from there -- consecutive lanes write consecutive words of a bucket's range;
//   histogram  weigh_streams_kernel's inner loop over the work list: an item is one team's share of one bucket's
//            tiles and one row of the slab.  A workgroup takes items b, b + G, ..: nothing rests on having as many
//            workgroups as non-empty buckets;
//   merge    weigh_merge_kernel reads a bucket's rows [item_first[k], item_first[k + 1]) from the same table.
//
// The partition costs one more read and write of the records; its time does not depend on where a sample's hot
// subjects sit.  (Atomics into a W[n_subjects] array in HBM would serialise a sample whose hot subjects share a few
// addresses.)  Results are exact integers and never depend on launch shape or atomic order: which slot of a bucket's
// range a word lands in is free, what is added to a bin is not.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include "wk_weigh.hpp"
#define WK_WIDE_FN __host__ __device__ __forceinline__
#else
#define WK_WIDE_FN inline
#endif

namespace wk {

constexpr uint32_t kWideSubjBits = 23;                     // subject index of a packed word (kWordSubjBits)
constexpr uint32_t kWideBins = 40608;                      // subjects per bucket (kSliceBins)
constexpr uint32_t kWideMaxBuckets = ((1u << kWideSubjBits) + kWideBins - 1u) / kWideBins;   // 207
constexpr uint32_t kWideMaxWgs = 1024;                     // workgroups of the histogram, at most
constexpr uint32_t kWideMaxItems = kWideMaxWgs + kWideMaxBuckets;
constexpr uint32_t kWideAlign = 4;                         // a bucket's records start at a multiple of 4 words (16-byte loads)
#if defined(__HIPCC__)
static_assert(kWideSubjBits == kWordSubjBits && kWideBins == kSliceBins, "the wide layout cuts the table as the streams do");
#endif

// the bucket of a packed word among n_buckets >= 1
WK_WIDE_FN uint32_t wide_bucket(uint32_t word, uint32_t n_buckets) {
    const uint32_t b = (word & ((1u << kWideSubjBits) - 1u)) / kWideBins;
    return b < n_buckets ? b : n_buckets - 1u;
}

// What the scan leaves in HBM for the scatter, the histogram and the merge.
struct WidePlan {
    uint32_t n_items, n_buckets;
    uint32_t start[kWideMaxBuckets + 1];       // bucket k's records: [start[k], start[k] + count[k]) of the second buffer
    uint32_t count[kWideMaxBuckets];
    uint32_t item_first[kWideMaxBuckets + 1];  // items (= slab rows) [item_first[k], item_first[k + 1]) walk bucket k
    uint32_t item_bucket[kWideMaxItems];
};

// words the second buffer needs for n records, whatever their buckets
WK_WIDE_FN uint64_t wide_room(uint64_t n_records) { return n_records + (uint64_t)(kWideAlign - 1u) * kWideMaxBuckets + kWideAlign; }

// Workgroups in proportion to the buckets' lengths: with q = ceil(total / n_wg) records as a workgroup's fair share,
// bucket k is walked by ceil(count[k] / q) items of at most q records each -- at most n_wg + (non-empty buckets)
// items in all, none for an empty bucket.  Needs total < 2^31, 1 <= n_buckets <= kWideMaxBuckets, 1 <= n_wg <=
// kWideMaxWgs.
WK_WIDE_FN void wide_plan(const uint32_t* counts, uint32_t n_buckets, uint32_t n_wg, WidePlan* p) {
    uint32_t total = 0;
    for (uint32_t k = 0; k < n_buckets; ++k) total += counts[k];
    uint32_t q = (total + n_wg - 1u) / n_wg;
    if (q == 0u) q = 1u;
    uint32_t pos = 0, items = 0;
    for (uint32_t k = 0; k < n_buckets; ++k) {
        const uint32_t n = counts[k];
        p->start[k] = pos;
        p->count[k] = n;
        p->item_first[k] = items;
        const uint32_t teams = (n + q - 1u) / q;
        for (uint32_t t = 0; t < teams; ++t) p->item_bucket[items++] = k;
        pos += (n + kWideAlign - 1u) & ~(kWideAlign - 1u);
    }
    p->start[n_buckets] = pos;
    p->item_first[n_buckets] = items;
    p->n_items = items;
    p->n_buckets = n_buckets;
}

#if defined(__HIPCC__)

constexpr uint32_t kWideThreads = 1024;
constexpr uint32_t kWideItems = 8;                            // words per thread and tile: two 16-byte loads
constexpr uint32_t kWideTile = kWideThreads * kWideItems;     // 8 192 words per workgroup and round
constexpr uint32_t kWideCursorPad = 32;                       // a bucket's cursor has a 128-byte line of its own
constexpr uint32_t kWideNone = 0xFFFFFFFFu;

// a tile's words of this thread (words past the end: none) and their buckets
struct WideTile {
    uint32_t word[kWideItems], bucket[kWideItems];
};
__device__ __forceinline__ WideTile wide_load(const __amdgpu_buffer_rsrc_t& rsrc, uint32_t tile, uint32_t n, uint32_t n_buckets) {
    WideTile t;
#pragma unroll
    for (uint32_t h = 0; h < kWideItems / 4u; ++h) {
        const uint32_t i = tile * kWideTile + (h * kWideThreads + threadIdx.x) * 4u;  // (tile * kWideTile < n < 2^30)
        const v4i32 x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(i << 2), 0, 0);  // (zeros past the end)
        const uint32_t w[4] = {(uint32_t)x.x, (uint32_t)x.y, (uint32_t)x.z, (uint32_t)x.w};
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            t.word[h * 4u + j] = w[j];
            t.bucket[h * 4u + j] = i + j < n ? wide_bucket(w[j], n_buckets) : kWideNone;
        }
    }
    return t;
}
// words of a tile (the last one may be short)
__device__ __forceinline__ uint32_t wide_tile_len(uint32_t tile, uint32_t n) { return min(kWideTile, n - tile * kWideTile); }

// One add per lane on an LDS counter, the lanes that name the first lane's bucket -- nearly all of them where a
// sample's records sit in one hot bucket -- served by a single add: returns the counter's value in front of this
// lane's add (its rank among the tile's words of the bucket).  Every lane of the wave calls.
__device__ __forceinline__ uint32_t wide_take(uint32_t* cnt, uint32_t b) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t hot = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    const bool same = b == hot;
    const unsigned long long m = __ballot(same);
    uint32_t at = 0;
    if (lane == 0) {
        if (hot != kWideNone) at = atomicAdd(&cnt[hot], (uint32_t)__popcll(m));
    } else if (!same && b != kWideNone) {
        at = atomicAdd(&cnt[b], 1u);
    }
    const uint32_t first = (uint32_t)__shfl((int)at, 0, kWave);
    return same ? first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) : at;
}

// ---- count --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWideThreads) wide_count_kernel(const uint32_t* __restrict__ words, uint32_t n, uint32_t n_buckets,
                                                                  uint32_t* __restrict__ bucket_count) {
    __shared__ uint32_t cnt[kWideMaxBuckets + 1];
    if (threadIdx.x <= kWideMaxBuckets) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(words), 0, (int)(n << 2), 0x00020000);
    const uint32_t n_tiles = (n + kWideTile - 1u) / kWideTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const WideTile t = wide_load(rsrc, tile, n, n_buckets);
#pragma unroll
        for (uint32_t r = 0; r < kWideItems; ++r) (void)wide_take(cnt, t.bucket[r]);
    }
    __syncthreads();
    if (threadIdx.x < n_buckets && cnt[threadIdx.x]) atomicAdd(&bucket_count[threadIdx.x], cnt[threadIdx.x]);
}

// ---- scan ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wide_scan_kernel(const uint32_t* __restrict__ bucket_count, uint32_t n_buckets, uint32_t n_wg,
                                                        WidePlan* plan, uint32_t* __restrict__ cursor) {
    __shared__ uint32_t counts[kWideMaxBuckets];
    if (threadIdx.x < n_buckets) counts[threadIdx.x] = bucket_count[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) wide_plan(counts, n_buckets, n_wg, plan);
    __threadfence();
    __syncthreads();
    if (threadIdx.x < n_buckets) cursor[threadIdx.x * kWideCursorPad] = plan->start[threadIdx.x];
}

// ---- scatter ------------------------------------------------------------------------------------------------
// `out` holds `cap` words; nothing is stored at or beyond cap whatever the cursors say.
__global__ void __launch_bounds__(kWideThreads) wide_scatter_kernel(const uint32_t* __restrict__ words, uint32_t n, uint32_t n_buckets,
                                                                    uint32_t* __restrict__ cursor, uint32_t* __restrict__ out, uint32_t cap) {
    __shared__ uint32_t cnt[256], lstart[256], gbase[256], wsum[4];
    __shared__ uint32_t image[kWideTile];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(words), 0, (int)(n << 2), 0x00020000);
    const uint32_t n_tiles = (n + kWideTile - 1u) / kWideTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (threadIdx.x < 256u) cnt[threadIdx.x] = 0u;
        __syncthreads();
        const WideTile t = wide_load(rsrc, tile, n, n_buckets);
        uint32_t rank[kWideItems];
#pragma unroll
        for (uint32_t r = 0; r < kWideItems; ++r) rank[r] = wide_take(cnt, t.bucket[r]);
        __syncthreads();
        // the buckets' starts in the image (exclusive scan of the counters, a bucket per thread of the first four
        // waves) and in the second buffer (one reservation per non-empty bucket)
        uint32_t c = 0, incl = 0;
        if (threadIdx.x < 256u) {
            c = cnt[threadIdx.x];
            incl = c;
#pragma unroll
            for (uint32_t off = 1; off < (uint32_t)kWave; off <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, off, kWave);
                if (lane >= off) incl += up;
            }
            if (lane == (uint32_t)kWave - 1u) wsum[wave] = incl;
        }
        __syncthreads();
        if (threadIdx.x < 256u) {
            uint32_t before = 0;
            for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
            lstart[threadIdx.x] = before + incl - c;
            gbase[threadIdx.x] = c ? atomicAdd(&cursor[threadIdx.x * kWideCursorPad], c) : 0u;  // (c > 0: a bucket < n_buckets)
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < kWideItems; ++r)
            if (t.bucket[r] != kWideNone) image[lstart[t.bucket[r]] + rank[r]] = t.word[r];
        __syncthreads();
        const uint32_t len = wide_tile_len(tile, n);
        for (uint32_t i = threadIdx.x; i < len; i += kWideThreads) {
            const uint32_t w = image[i];
            const uint32_t b = wide_bucket(w, n_buckets);
            const uint32_t at = gbase[b] + (i - lstart[b]);
            if (at < cap) out[at] = w;
        }
        // (the next round's first stores to lstart, gbase and image lie behind barriers every thread passes after this loop)
    }
}

// ---- histogram ----------------------------------------------------------------------------------------------
struct WideBinsArgs {
    const uint32_t* words;   // the second buffer
    const WidePlan* plan;
    uint32_t n_subjects;
    uint32_t* slab;          // [slab_rows][kSliceBins], a row per item
    uint32_t slab_rows;
    uint32_t* hi;            // [n_subjects]
    int* err;
};

template <int kRing = 4>
__global__ void __launch_bounds__(kWeighThreads) weigh_wide_kernel(WideBinsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t lut[32];
    uint32_t* bins = reinterpret_cast<uint32_t*>(smem);
    if (threadIdx.x < 32u)
        lut[threadIdx.x] = (threadIdx.x >= 1u && threadIdx.x <= (uint32_t)WK_WEIGHT_MAX_K) ? weight_of(threadIdx.x) : 0u;
    const WidePlan* __restrict__ plan = a.plan;
    const uint32_t n_items = min(plan->n_items, min(a.slab_rows, kWideMaxItems));
    const uint32_t idle_addr = kSliceBins + (threadIdx.x & 63u);
    bool outside = false;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t k = min(plan->item_bucket[item], kWideMaxBuckets - 1u);
        const uint32_t first = plan->item_first[k];
        const uint32_t team = item - first, n_teams = plan->item_first[k + 1] - first;
        const uint32_t lo = k * kSliceBins;
        const uint32_t span = min(kSliceBins, a.n_subjects - min(lo, a.n_subjects));
        const uint32_t n_records = plan->count[k];

        for (uint32_t i = threadIdx.x; i < kSliceBins + 64u; i += kWeighThreads) bins[i] = 0u;
        __syncthreads();

        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.words + plan->start[k]), 0, (int)(n_records << 2), 0x00020000);
        const uint32_t n_tiles = (n_records + kBinsTile - 1u) / kBinsTile;
        v4i32 ring[kRing];
        auto load = [&](uint32_t tile, v4i32& x) {
            const uint32_t i = tile * kBinsTile + threadIdx.x * 4u;
            x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(tile < n_tiles ? i << 2 : 0xFFFFFFF0u), 0, 0);
        };
        auto add = [&](const v4i32& x) {
            uint32_t c[4] = {(uint32_t)x.x, (uint32_t)x.y, (uint32_t)x.z, (uint32_t)x.w};
            uint32_t w[4], at[4], old[4];
            bool in[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[j] = lut[c[j] >> kWordSizeShift];  // (past the end: 0, weight 0)
                c[j] &= kWordSubjMask;
                const uint32_t idx = c[j] - lo;
                in[j] = idx < span;
                outside |= (w[j] != 0u) & !in[j];
                at[j] = in[j] ? idx : idle_addr;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) old[j] = atomicAdd(&bins[at[j]], w[j]);
            bool wrapped = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) wrapped |= in[j] & (old[j] + w[j] < old[j]);
            if (wrapped) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in[j] & (old[j] + w[j] < old[j])) atomicAdd(&a.hi[c[j]], 1u);
            }
        };
        uint32_t tile = team;
#pragma unroll
        for (int u = 0; u < kRing - 1; ++u) load(tile + (uint32_t)u * n_teams, ring[u]);
        while (tile < n_tiles) {
#pragma unroll
            for (int u = 0; u < kRing; ++u) {
                load(tile + (uint32_t)(kRing - 1) * n_teams, ring[(u + kRing - 1) % kRing]);
                add(ring[u]);
                tile += n_teams;
            }
        }
        __syncthreads();
        uint32_t* row = a.slab + (size_t)item * kSliceBins;
        for (uint32_t i = threadIdx.x; i < span; i += kWeighThreads) row[i] = bins[i];
        __syncthreads();  // (the bins are cleared for the next item)
    }
    if (outside) atomicOr(a.err, kErrFeatureRange);
}

#endif  // __HIPCC__

}  // namespace wk
