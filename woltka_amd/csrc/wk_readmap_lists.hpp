// wk_readmap_lists.hpp — the read maps of `--outmap` with taxon lists, formatted on the device.
//
// A read a job splits over several features (`none` without --uniq, a plain rank without --uniq / --above /
// --major: classify.assign_none / assign_rank, classify.py:32-51, 81-127) carries the code WK_ASSIGN_MULTI, and
// file.write_readmap (file.py:469-500) prints `query[/mate] <tab> taxon:count <tab> taxon:count ...` for it: the
// read's distinct subjects, each mapped to its feature (none) or its ancestor at the job's rank (subjects without
// one, or outside the hierarchy, are dropped), counted per feature and ordered by count descending, then by the
// feature id's bytes ascending (UTF-8 byte order is Python's string order).  --unassigned does not touch a list.
// Every other code is printed as wk_readmap_reads.hpp prints it.  The block is the staged chunk of
// wk_dtok_stage_reads_plain with the codes wk_classify_staged_keep left; the subjects of a read are the CSR span
// [qoff[r], qoff[r + 1]) of subject indices, subj_feat names their features, `anc` is the rank table
// classify_kernel reads for the job.
//
// Kernels, per job:
//   readmap_lists_build  a workgroup per tile of kDtokThreads reads.  A thread per read with a single code: its
//                        line's length (readmap_reads_line_len).  A wave per list of up to 64 subjects, a lane
//                        per subject, all in registers: duplicates and groups by comparing against every lane
//                        (__shfl), an element's place = the group leaders that sort before it.  The workgroup per
//                        list of up to WK_MAX_K subjects: three bitonic sorts in LDS (subjects, features,
//                        (count, id)).  The sorted (feature, count) pairs go to pairs[qoff[r] ...] -- a read has
//                        at most as many features as subjects --, their number to n_pairs[r], the line's length
//                        to read_len[r].
//   u64_tile_*           the scan of the lengths (wk_readmap.hpp)
//   readmap_lists_write  a thread per read with a single code (readmap_reads_write_line), a wave per list: the
//                        pieces' places from a wave prefix sum, 64 pairs a round.
//
// Limits: WK_ASSIGN_EMPTY, a feature or subject outside the tables, a list of no feature or of more than
// WK_MAX_K subjects raise kReadsBadCode: the caller gives no text then.  Nothing is written past out_cap.
#pragma once
#include "wk_readmap_reads.hpp"

namespace wk {

constexpr uint32_t kListsLds = 4096;  // elements the workgroup sorts: WK_MAX_K subjects and a pad
static_assert(WK_MAX_K < kListsLds, "a list's subjects must fit the LDS arrays");
constexpr uint32_t kListsPad = 0xFFFFFFFFu;

struct ReadmapListsArgs {
    ReadmapReadsArgs m;
    const int32_t* subj;             // [n_records] subject indices, read by read
    const int32_t* qoff;             // [n_reads + 1]
    const int32_t* subj_feat;        // [n_subjects] feature of a subject
    uint32_t n_subjects;
    const int32_t* anc;              // [n_nodes] ancestor at the job's rank or -1; null: the feature itself (none)
    uint32_t n_nodes;
    const uint32_t* key_off;         // [n_shown + 1] the bytes the lists are ordered by: the feature ids
    const unsigned char* key;
    uint2* pairs;                    // [n_records] (feature, count) of the lists, at the read's first record
    uint32_t* n_pairs;               // [n_reads]
};

// id bytes of feature x < those of feature y
__device__ __forceinline__ bool lists_id_less(const ReadmapListsArgs& L, uint32_t x, uint32_t y) {
    const uint32_t xo = L.key_off[x], xn = L.key_off[x + 1] - xo;
    const uint32_t yo = L.key_off[y], yn = L.key_off[y + 1] - yo;
    const uint32_t n = xn < yn ? xn : yn;
    for (uint32_t k = 0; k < n; ++k) {
        const unsigned char p = L.key[xo + k], q = L.key[yo + k];
        if (p != q) return p < q;
    }
    return xn < yn;
}

// The feature subject s stands for in this job's list: -1 = dropped.
__device__ __forceinline__ int32_t lists_feature(const ReadmapListsArgs& L, int32_t s) {
    if ((uint32_t)s >= L.n_subjects) {
        atomicOr(L.m.flags, kReadsBadCode);
        return -1;
    }
    int32_t f = L.subj_feat[s];
    if (L.anc) f = (f >= 0 && (uint32_t)f < L.n_nodes) ? L.anc[f] : -1;
    if (f < 0) return -1;
    if ((uint32_t)f >= L.m.n_shown) {
        atomicOr(L.m.flags, kReadsBadCode);
        return -1;
    }
    return f;
}

// bytes of `<tab>shown:count`
__device__ __forceinline__ uint32_t lists_piece_len(const ReadmapListsArgs& L, uint32_t t, uint32_t count) {
    return 2u + (L.m.shown_off[t + 1] - L.m.shown_off[t]) + dec_digits(count);
}

// The line of list r with `pieces` bytes of pairs (lane 0 / thread 0 of the read's team)
template <bool kDemux = false>
__device__ __forceinline__ void lists_set_len(const DtokArgs& a, const ReadmapListsArgs& L, uint32_t r, uint32_t n_pairs,
                                              unsigned long long pieces) {
    const uint32_t i = L.m.read_line[r];
    unsigned long long len = 0;
    if (n_pairs == 0) {
        atomicOr(L.m.flags, kReadsBadCode);  // (a list holds two values that differ: one of them is a feature)
    } else if (i < a.n_lines) {
        const ReadmapId id = readmap_id<kDemux>(a, i);
        len = (unsigned long long)id.n + (id.mate ? 2u : 0u) + pieces + 1u;
    } else {
        n_pairs = 0;  // (a read no leader names has no line, as with a single code)
    }
    L.n_pairs[r] = n_pairs;
    L.m.read_len[r] = len;
}

// A wave builds the list of read r: n <= 64 subjects from record lo on, one per lane.
template <bool kDemux = false>
__device__ __forceinline__ void lists_wave_build(const DtokArgs& a, const ReadmapListsArgs& L, uint32_t r, int32_t lo, int32_t n,
                                                 uint32_t lane) {
    const bool mine = (int32_t)lane < n;
    const int32_t s = mine ? L.subj[lo + lane] : -1;
    bool dup = false;
    for (int32_t j = 0; j < n; ++j) {
        const int32_t sj = __shfl(s, j, kWave);
        dup |= j < (int32_t)lane && sj == s;
    }
    const int32_t t = (mine && !dup) ? lists_feature(L, s) : -1;
    uint32_t count = 0;
    bool head = t >= 0;
    for (int32_t j = 0; j < n; ++j) {
        const int32_t tj = __shfl(t, j, kWave);
        if (tj == t) {
            count += 1u;
            if (j < (int32_t)lane) head = false;
        }
    }
    const unsigned long long heads = __ballot(head);
    uint32_t place = 0;
    for (unsigned long long todo = heads; todo; todo &= todo - 1ull) {
        const int j = __ffsll((long long)todo) - 1;
        const uint32_t cj = __shfl(count, j, kWave);
        const int32_t tj = __shfl(t, j, kWave);
        if (head && j != (int)lane && (cj > count || (cj == count && lists_id_less(L, (uint32_t)tj, (uint32_t)t)))) place += 1u;
    }
    if (head) L.pairs[lo + place] = make_uint2((uint32_t)t, count);
    const unsigned long long pieces = wave_sum(head ? (unsigned long long)lists_piece_len(L, (uint32_t)t, count) : 0ull);
    if (lane == 0) lists_set_len<kDemux>(a, L, r, (uint32_t)__popcll(heads), pieces);
}

// Bitonic sort of key[0, m2), m2 a power of two, by the whole workgroup (which has met at a barrier).
template <typename Less>
__device__ __forceinline__ void lists_bitonic(unsigned long long* key, uint32_t m2, Less less) {
    for (uint32_t k = 2; k <= m2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < m2; i += kDtokThreads) {
                const uint32_t p = i ^ j;
                if (p > i) {
                    const unsigned long long x = key[i], y = key[p];
                    if ((i & k) == 0 ? less(y, x) : less(x, y)) {
                        key[i] = y;
                        key[p] = x;
                    }
                }
            }
            __syncthreads();
        }
}

// The workgroup builds the list of read r: 64 < n <= WK_MAX_K subjects from record lo on.
template <bool kDemux = false>
__device__ __forceinline__ void lists_block_build(const DtokArgs& a, const ReadmapListsArgs& L, uint32_t r, int32_t lo, int32_t n,
                                                  unsigned long long* key, uint32_t* aux, unsigned long long* red) {
    const uint32_t tid = threadIdx.x;
    uint32_t m2 = 128;
    while (m2 < (uint32_t)n) m2 <<= 1;
    const auto plain = [](unsigned long long x, unsigned long long y) { return x < y; };
    // the subjects in order: duplicates are neighbours
    for (uint32_t k = tid; k < m2; k += kDtokThreads) key[k] = k < (uint32_t)n ? (unsigned long long)(uint32_t)L.subj[lo + k] : (unsigned long long)kListsPad;
    __syncthreads();
    lists_bitonic(key, m2, plain);
    for (uint32_t k = tid; k < m2; k += kDtokThreads) {
        int32_t t = -1;
        if (k < (uint32_t)n && (k == 0 || key[k] != key[k - 1])) t = lists_feature(L, (int32_t)(uint32_t)key[k]);
        aux[k] = t < 0 ? kListsPad : (uint32_t)t;
    }
    __syncthreads();
    // the features in order: a feature's subjects are a run
    for (uint32_t k = tid; k < m2; k += kDtokThreads) key[k] = aux[k];
    __syncthreads();
    lists_bitonic(key, m2, plain);
    for (uint32_t k = tid; k < m2; k += kDtokThreads) {
        const unsigned long long t = key[k];
        uint32_t count = 0;
        if (t != kListsPad && (k == 0 || key[k - 1] != t)) {
            uint32_t b = k, e = m2;  // the first element behind the run
            while (b + 1u < e) {
                const uint32_t mid = (b + e) >> 1;
                if (key[mid] == t)
                    b = mid;
                else
                    e = mid;
            }
            count = e - k;
        }
        aux[k] = count;
    }
    __syncthreads();
    // the runs' heads by (count descending, id): the others go behind them
    for (uint32_t k = tid; k < m2; k += kDtokThreads)
        key[k] = aux[k] ? ((unsigned long long)((uint32_t)WK_MAX_K - aux[k]) << 32) | key[k] : ~0ull;
    __syncthreads();
    lists_bitonic(key, m2, [&L](unsigned long long x, unsigned long long y) {
        const uint32_t hx = (uint32_t)(x >> 32), hy = (uint32_t)(y >> 32);
        if (hx != hy) return hx < hy;
        if (x == y || hx == kListsPad) return false;
        return lists_id_less(L, (uint32_t)x, (uint32_t)y);
    });
    unsigned long long mine = 0;  // bytes of this thread's pieces, and their number above bit 40
    for (uint32_t k = tid; k < m2; k += kDtokThreads) {
        const unsigned long long e = key[k];
        if (e == ~0ull) continue;
        const uint32_t t = (uint32_t)e, count = (uint32_t)WK_MAX_K - (uint32_t)(e >> 32);
        if (k < (uint32_t)n) L.pairs[lo + k] = make_uint2(t, count);
        mine += (unsigned long long)lists_piece_len(L, t, count) + (1ull << 40);
    }
    mine = wave_sum(mine);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = mine;
    __syncthreads();
    if (tid == 0) {
        unsigned long long all = 0;
        for (uint32_t w = 0; w < kDtokThreads / kWave; ++w) all += red[w];
        lists_set_len<kDemux>(a, L, r, (uint32_t)(all >> 40), all & ((1ull << 40) - 1ull));
    }
    __syncthreads();
}

// The tile of blockIdx.x.  kDemux: the read part of the id is printed, and a read whose sample the whitelist drops
// (samp[r] < 0) has no line (wk_readmap_demux.hpp).
template <bool kDemux>
__device__ __forceinline__ void lists_build_tile(const DtokArgs& a, const ReadmapListsArgs& L, const int32_t* __restrict__ samp) {
    __shared__ unsigned long long key[kListsLds];
    __shared__ uint32_t aux[kListsLds];
    __shared__ unsigned long long red[kDtokThreads / kWave];
    __shared__ uint32_t big[kDtokThreads];  // the tile's lists of more than 64 subjects
    __shared__ uint32_t n_big;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t r = blockIdx.x * kDtokThreads + tid;
    if (tid == 0) n_big = 0;
    __syncthreads();
    int32_t lo = 0, n = 0;
    bool list = false;
    if (r < L.m.n_reads) {
        const int32_t v = L.m.assign[r];
        if (kDemux && samp[r] < 0) {
            L.n_pairs[r] = 0;
            L.m.read_len[r] = 0;
        } else if (v != WK_ASSIGN_MULTI) {
            L.m.read_len[r] = readmap_reads_line_len<kDemux>(a, L.m, r, v);
        } else {
            lo = L.qoff[r];
            n = L.qoff[r + 1] - lo;
            list = lo >= 0 && n >= 1 && n <= WK_MAX_K;
            if (!list) {
                atomicOr(L.m.flags, kReadsBadCode);
                L.n_pairs[r] = 0;
                L.m.read_len[r] = 0;
            }
        }
    }
    const bool large = list && n > kWave;
    if (large) big[atomicAdd(&n_big, 1u)] = tid;
    for (unsigned long long todo = __ballot(list && !large); todo; todo &= todo - 1ull) {
        const int src = __ffsll((long long)todo) - 1;
        lists_wave_build<kDemux>(a, L, r - lane + (uint32_t)src, __shfl(lo, src, kWave), __shfl(n, src, kWave), lane);
    }
    __syncthreads();
    const uint32_t todo_big = n_big;
    for (uint32_t b = 0; b < todo_big; ++b) {
        const uint32_t rb = blockIdx.x * kDtokThreads + big[b];
        const int32_t lb = L.qoff[rb];
        lists_block_build<kDemux>(a, L, rb, lb, L.qoff[rb + 1] - lb, key, aux, red);
    }
}

__global__ void __launch_bounds__(kDtokThreads) readmap_lists_build_kernel(DtokArgs a, ReadmapListsArgs L) {
    lists_build_tile<false>(a, L, nullptr);
}

// A wave writes the line of list r at read_len[r] (now the exclusive prefix, or the place the partition gave it).
template <bool kDemux = false>
__device__ __forceinline__ void lists_wave_write(const DtokArgs& a, const ReadmapListsArgs& L, uint32_t r, uint32_t lane) {
    const uint32_t n_pairs = L.n_pairs[r];
    const uint32_t i = L.m.read_line[r];
    if (n_pairs == 0 || i >= a.n_lines) return;
    unsigned long long at = L.m.read_len[r];
    const unsigned long long cap = L.m.out_cap;
    const ReadmapId id = readmap_id<kDemux>(a, i);
    const uint32_t qn = id.n, mate = id.mate ? a.lmeta[i] >> 28 : 0u;
    unsigned char* o = L.m.out;
    const unsigned char* q = a.text + id.off;
    for (uint32_t k = lane; k < qn; k += kWave)
        if (at + k < cap) o[at + k] = q[k];
    at += qn;
    if (mate) {
        if (lane == 0 && at + 2u <= cap) {
            o[at] = '/';
            o[at + 1] = (unsigned char)('0' + mate);
        }
        at += 2u;
    }
    const int32_t lo = L.qoff[r];
    for (uint32_t base = 0; base < n_pairs; base += kWave) {
        const bool has = base + lane < n_pairs;
        uint2 p = make_uint2(0u, 0u);
        uint32_t len = 0;
        if (has) {
            p = L.pairs[lo + base + lane];
            len = lists_piece_len(L, p.x, p.y);
        }
        uint32_t incl = len;  // inclusive prefix of the round's pieces
        for (uint32_t d = 1; d < (uint32_t)kWave; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += up;
        }
        unsigned long long w = at + (incl - len);
        if (has && w + len <= cap) {  // (the lengths said otherwise: nothing past the text)
            const unsigned char* s = L.m.shown + L.m.shown_off[p.x];
            const uint32_t sn = L.m.shown_off[p.x + 1] - L.m.shown_off[p.x];
            o[w++] = '\t';
            for (uint32_t k = 0; k < sn; ++k) o[w + k] = s[k];
            w += sn;
            o[w++] = ':';
            uint32_t v = p.y;
            for (uint32_t k = dec_digits(p.y); k-- > 0;) {
                o[w + k] = (unsigned char)('0' + v % 10u);
                v /= 10u;
            }
        }
        at += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0 && at < cap) o[at] = '\n';
}

template <bool kDemux>
__device__ __forceinline__ void lists_write_tile(const DtokArgs& a, const ReadmapListsArgs& L, const int32_t* __restrict__ samp) {
    const uint32_t r = blockIdx.x * kDtokThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    bool list = false;
    if (r < L.m.n_reads) {
        const int32_t v = L.m.assign[r];
        const bool drop = kDemux && samp[r] < 0;
        list = v == WK_ASSIGN_MULTI && !drop;
        if (!list && !drop) readmap_reads_write_line<kDemux>(a, L.m, r, v);
    }
    for (unsigned long long todo = __ballot(list); todo; todo &= todo - 1ull)
        lists_wave_write<kDemux>(a, L, r - lane + (uint32_t)(__ffsll((long long)todo) - 1), lane);
}

__global__ void __launch_bounds__(kDtokThreads) readmap_lists_write_kernel(DtokArgs a, ReadmapListsArgs L) {
    lists_write_tile<false>(a, L, nullptr);
}

}  // namespace wk
