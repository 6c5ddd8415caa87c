// wk_sized.hpp — size-normalised counts (`--sizes`) of the plain assigners from
// the packed records.
//
// classify.counter_size (woltka/classify.py:174-213) gives every one of the n
// subjects of a read sizes[sub] / n on taxon(sub) — whether the taxa of the
// read coincide (one taxon gets sum(sizes) / n, line 206) or not (each taxon
// gets sizes[sub] * (1 / n), line 212).  For the job sets the weighted histogram
// takes (wk_weigh.hpp: `--rank none` / `--rank <rank>` without --uniq / --major
// / --above, every subject with an ancestor at every rank, reads of <= 16
// subjects) the generic evaluator therefore logs one row {taxon_j(s),
// feature(s), j << 16 | n, group} per subject s of a read and job j
// (wk_classify.hpp, log_append), and the whole log of a sample is determined
// by the integer table
//
//     C[s][k] = number of records of subject s in reads of k subjects.
//
// A packed record carries both fields (subject in bits 0-22, read size in
// bits 27-31), so C is a histogram over the record streams:
//
//   sized_bins_kernel   C in LDS.  The kSliceBins bins of a workgroup are one
//                       *sub-slice* of kSizedSub consecutive subjects x 16 read
//                       sizes.  The workgroups of a team walk the same tiles
//                       of records, each adding 1 to the bin of the records of
//                       its sub-slice (one LDS add per record, no global
//                       atomic); every workgroup stores its bins as one slab
//                       row.
//   sized_rows_kernel   sums the slab rows of a sub-slice; <false>: counts the
//                       non-zero bins (the row buffer is sized from that
//                       number) and leaves the sums in the sub-slice's first
//                       row; <true>: one row per non-zero bin and job into the
//                       row buffer, appended per wave (ballot + one returning
//                       atomic, like log_append).
#pragma once
#include "wk_weigh.hpp"

namespace wk {

constexpr uint32_t kSizedSizes = WK_WEIGHT_MAX_K;             // read sizes 1..16
constexpr uint32_t kSizedSub = kSliceBins / kSizedSizes;      // subjects per sub-slice
static_assert(kSizedSizes == 16, "a packed record's read size is 1..16");
static_assert(kSizedSub * kSizedSizes == kSliceBins, "a slice of the streams is a whole number of sub-slices");
constexpr uint32_t kSizedThreads = 1024;
constexpr uint32_t kSizedTile = kSizedThreads * 4;            // records per workgroup and round

struct SizedBinsArgs {
    const uint32_t* words;  // one stream of packed records
    uint32_t n_records;
    uint32_t n_subjects;
    uint32_t q_first;       // first sub-slice of the subjects this stream holds
    uint32_t n_q;           // ... and how many
    uint32_t n_teams;
    uint32_t* slab;         // [n_q][n_teams][kSliceBins], the rows of this stream
    int* err;
};

template <int kRing = 4>
__global__ void __launch_bounds__(kSizedThreads) sized_bins_kernel(SizedBinsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* bins = reinterpret_cast<uint32_t*>(smem);
    // workgroup b runs on XCD b mod 8: with whole octets of teams the sub-slices
    // of a team share an XCD, whose L2 then serves the team's later readers
    uint32_t q, team;
    if (a.n_teams % 8u == 0u) {
        const uint32_t xcd = blockIdx.x % 8u, m = blockIdx.x / 8u;
        q = m % a.n_q;
        team = (m / a.n_q) * 8u + xcd;
    } else {
        q = blockIdx.x % a.n_q;
        team = blockIdx.x / a.n_q;
    }
    if (team >= a.n_teams) return;
    const uint32_t lo = (a.q_first + q) * kSizedSub;
    const uint32_t span = min(kSizedSub, a.n_subjects - min(lo, a.n_subjects));

    for (uint32_t i = threadIdx.x; i < kSliceBins; i += kSizedThreads) bins[i] = 0u;
    __syncthreads();

    // through a buffer resource: the range check returns zeros past the end
    // (size 0: no record), so the last round needs no special case
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.words), 0, (int)(a.n_records << 2), 0x00020000);
    const uint32_t n_tiles = (a.n_records + kSizedTile - 1u) / kSizedTile;
    v4i32 ring[kRing];
    auto load = [&](uint32_t tile, v4i32& x) {
        const uint32_t i = tile * kSizedTile + threadIdx.x * 4u;
        x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(tile < n_tiles ? i << 2 : 0xFFFFFFF0u), 0, 0);
    };
    bool outside = false;
    auto add = [&](const v4i32& x) {
        const uint32_t c[4] = {(uint32_t)x.x, (uint32_t)x.y, (uint32_t)x.z, (uint32_t)x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = c[j] >> kWordSizeShift;
            const uint32_t s = c[j] & kWordSubjMask;
            const uint32_t idx = s - lo;
            outside |= (k != 0u) & ((s >= a.n_subjects) | (k > kSizedSizes));
            // (nothing is read back: an add without a result, under the lanes' mask)
            if ((idx < span) & (k - 1u < kSizedSizes)) atomicAdd(&bins[idx * kSizedSizes + (k - 1u)], 1u);
        }
    };
    uint32_t tile = team;
#pragma unroll
    for (int u = 0; u < kRing - 1; ++u) load(tile + (uint32_t)u * a.n_teams, ring[u]);
    while (tile < n_tiles) {
#pragma unroll
        for (int u = 0; u < kRing; ++u) {  // stages addressed by code position; steps past the end add nothing
            load(tile + (uint32_t)(kRing - 1) * a.n_teams, ring[(u + kRing - 1) % kRing]);
            add(ring[u]);
            tile += a.n_teams;
        }
    }
    if (outside) atomicOr(a.err, kErrFeatureRange);
    __syncthreads();
    uint32_t* row = a.slab + ((size_t)q * a.n_teams + team) * kSliceBins;
    for (uint32_t i = threadIdx.x; i < kSliceBins; i += kSizedThreads) row[i] = bins[i];
}

struct SizedRowsArgs {
    uint32_t* slab;
    uint32_t n_subjects;
    uint32_t sliced;                   // a stream per kSizedSizes sub-slices, or one stream for all of them
    uint32_t teams[kMaxStreams];       // slab rows per sub-slice of stream k (0: the stream holds no records)
    uint32_t row_first[kMaxStreams];   // first slab row of stream k
    const int32_t* rows;               // [n_subjects][row_w] = {feature, ancestor at rank column 0, 1, ...}
    int32_t row_w;
    int32_t n_jobs;
    int32_t mode[WK_MAX_JOBS];
    int32_t col[WK_MAX_JOBS];
    int32_t group;
    unsigned long long* n_bins;        // <false>: += non-zero bins
    int4* out_rows;                    // <true>: {feature_j(s), feature(s), j << 16 | k, group} ...
    long long* out_counts;             // ... and C[s][k]
    unsigned long long* cursor;        // rows appended by this launch
    unsigned long long base, cap;      // they go to [base, cap)
    int* err;
};

constexpr uint32_t kSizedRowsThreads = 256;
// grid: x over the bins of a sub-slice, y = sub-slice
template <bool kEmit>
__global__ void __launch_bounds__(kSizedRowsThreads) sized_rows_kernel(SizedRowsArgs a) {
    const uint32_t q = blockIdx.y;
    const uint32_t b = blockIdx.x * kSizedRowsThreads + threadIdx.x;
    const uint32_t k_stream = a.sliced ? q / kSizedSizes : 0u;
    const uint32_t q_in = a.sliced ? q % kSizedSizes : q;
    const uint32_t teams = a.teams[k_stream];
    const uint32_t s = q * kSizedSub + b / kSizedSizes;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint32_t v = 0;
    if (b < kSliceBins && s < a.n_subjects && teams) {
        uint32_t* p = a.slab + ((size_t)a.row_first[k_stream] + (size_t)q_in * teams) * kSliceBins + b;
        if constexpr (kEmit) {
            v = *p;  // (summed by the counting launch)
        } else {
#pragma unroll 4
            for (uint32_t t = 0; t < teams; ++t) v += p[(size_t)t * kSliceBins];
            if (teams > 1u) *p = v;
        }
    }
    const unsigned long long mask = __ballot(v != 0u);
    if (!mask) return;
    if constexpr (!kEmit) {
        if (lane == 0) atomicAdd(a.n_bins, (unsigned long long)__popcll(mask));
    } else {
        const int leader = __ffsll((long long)mask) - 1;
        unsigned long long at = 0;
        if ((int)lane == leader) at = atomicAdd(a.cursor, (unsigned long long)__popcll(mask) * (unsigned long long)a.n_jobs);
        at = __shfl(at, leader, kWave);
        if (v == 0u) return;
        at += a.base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull)) * (unsigned long long)a.n_jobs;
        const int32_t* row = a.rows + (size_t)s * a.row_w;
        const int32_t k = (int32_t)(b % kSizedSizes) + 1;
        for (int jb = 0; jb < a.n_jobs; ++jb) {
            const int32_t f = a.mode[jb] == WK_MODE_NONE ? row[0] : row[1 + a.col[jb]];
            if (f < 0 || (uint32_t)f > (uint32_t)WK_MAX_FEATURE) atomicOr(a.err, kErrFeatureRange);  // (cannot happen: such subjects are flagged)
            if (at + (unsigned long long)jb < a.cap) {
                a.out_rows[at + jb] = make_int4(f, row[0], (jb << 16) | k, a.group);
                a.out_counts[at + jb] = (long long)v;
            } else {
                atomicOr(a.err, kErrFeatureRange);  // (cannot happen: the buffer was sized from the count)
            }
        }
    }
}

}  // namespace wk
