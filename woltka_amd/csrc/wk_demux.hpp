// wk_demux.hpp — demultiplexing on the device: the sample of every read from its id.
//
// workflow.demultiplex (woltka/workflow.py:886-907) cuts every read id at its first
// '_': `left, _, right = query.partition('_')`, the sample is `left` when `right` is
// not empty and '' otherwise -- the read id being QNAME + ("/1" | "/2" for a mate), so
// that "S1_" is sample '' unpaired and sample "S1" as a mate.  A whitelist (`--samples`)
// drops the reads of every other sample.  The host tokenizer does this per read
// (wk_tokenize.cpp, tokenize_range); here the blocks the device tokenizer has scanned
// (wk_dtok.hpp, plain flavour) get their reads' samples without leaving the device:
//
//   table      an open-addressing table of the samples met so far, keyed by the 64-bit
//              NameHash of the name (wk_strata.hpp); the names' bytes in an arena.  Equal
//              hashes are told apart by their bytes: a mismatch continues the probe.  The
//              host builds it (wk_demux_register) from the names the kernels list.
//   lookup     a thread per line that leads a run: which of the run's two readings (mate
//              0, mate 1 | 2 -- they differ only for an id that ends in its first '_')
//              has a read that is emitted, and is that reading's name in the table?
//   interning  a name the table does not hold is claimed in the block's pending table:
//              a compare-and-swap on the hash elects the slot, a running minimum keeps
//              the first (line, reading) that brought the name.  A second kernel compares
//              every claimant's bytes with the winner's; a name that only shares the hash
//              moves on to the next slot and claims again (one round per such name: never
//              with honest 64-bit hashes, by design with the tests' `demux_hash_mask`).
//   placement  behind dtok_first / the line scan: every first line of a read writes its
//              subject to the CSR chunk the general evaluator counts (wk_classify.hpp), a
//              read's first record its offset, its sample's group and the sample's "met"
//              byte (demux_place_reads_kernel).
//
//   coord-match  behind a scan of the "ex" flavour the lookup asks only for readings that have a hit; the hits are
//              staged with a group per read (demux_place_hits_kernel) and matched like any staged chunk; the "met"
//              bytes are stored behind the match, for the reads that matched a gene (demux_met_hits_kernel).
//
// Limits: at most kDemuxMaxSamples samples (the table is half full then); a block that
// would bring more is left to the host tokenizer (kDemuxFull).
#pragma once
#include "wk_dtok.hpp"
#include "wk_strata.hpp"

namespace wk {

constexpr uint32_t kDemuxMaxSamples = 1u << 16;
constexpr uint32_t kDemuxSlots = 2u * kDemuxMaxSamples;  // load factor <= 1/2
constexpr uint32_t kDemuxAtSlot = 1u << 30;              // lsamp[]: the entry sits in pending slot (value & (kDemuxSlots - 1)), not verified yet

constexpr uint32_t kDemuxFull = 1;     // more distinct samples than the table holds
constexpr uint32_t kDemuxMissing = 2;  // (placement) a read whose sample the table does not hold: its names were not registered

struct DemuxSlot {
    unsigned long long hash;  // 0: empty
    uint32_t id;
    uint32_t pad;
};

struct DemuxPend {
    unsigned long long hash;  // 0: empty
    uint32_t inv;             // ~(2 * line + reading) of the first claimant, kept by atomicMax (0: none yet)
    uint32_t pad;
};

struct DemuxArgs {
    const DemuxSlot* tab;      // [kDemuxSlots]
    const uint2* name_off;     // [n samples] (offset, length) in the arena
    const unsigned char* arena;
    const int32_t* group;      // [n samples] (sample, no stratum) group, -1: outside the whitelist
    unsigned char* met;        // [n samples]
    DemuxPend* pend;           // [kDemuxSlots]
    uint32_t* pend_list;       // [kDemuxMaxSamples] pending slots in the order they were claimed
    uint32_t* state;           // [0] flags [1] pending names [2] entries that claim again
    int32_t* lsamp;            // [2 * n_lines] per (line, reading): -1 settled, a slot to start probing at, or slot | kDemuxAtSlot
    unsigned long long hash_mask;  // (tests) AND-ed into every hash, 0: none
    uint32_t max_new;          // names the table still takes
    // the CSR chunk
    int32_t* c_subj;
    int32_t* c_qoff;
    int32_t* c_group;
    uint32_t cap;              // records / reads the arrays hold
};

struct DemuxName {
    uint32_t off, len;
};

// the sample of the run led by `line`, read as mate 0 (reading 0) or as a mate (reading 1)
__device__ __forceinline__ DemuxName demux_sample(const DtokArgs& a, uint32_t line, uint32_t reading) {
    const uint32_t lo = a.line_start[line], qn = a.lmeta[line] & 0x0FFFFFFFu;
    uint32_t u = qn;
    for (uint32_t k = 0; k < qn; ++k)
        if (a.text[lo + k] == '_') {
            u = k;
            break;
        }
    if (u < qn && (u + 1u < qn || reading != 0u)) return DemuxName{lo, u};
    return DemuxName{lo, 0u};
}

// the hash a name goes by in the sample table and the pending table, never 0 (an empty slot); the host files the names
// it registers with the same two functions
__host__ __device__ __forceinline__ unsigned long long demux_hash_of(unsigned long long hash_mask, const unsigned char* p, uint32_t n) {
    NameHash nh;
    for (uint32_t k = 0; k < n; ++k) nh.put(p[k]);
    unsigned long long h = nh.done();
    if (hash_mask) h &= hash_mask;
    return h ? h : 1ull;
}

__device__ __forceinline__ unsigned long long demux_hash(const DemuxArgs& d, const unsigned char* p, uint32_t n) {
    return demux_hash_of(d.hash_mask, p, n);
}

__host__ __device__ __forceinline__ uint32_t demux_home(unsigned long long h) { return (uint32_t)(h ^ (h >> 32)) & (kDemuxSlots - 1u); }

// the id of the sample p[0, n) in the table, -1 if it is not there
__device__ __forceinline__ int32_t demux_find(const DemuxArgs& d, const unsigned char* p, uint32_t n, unsigned long long h) {
    uint32_t q = demux_home(h);
    for (uint32_t tries = 0; tries < kDemuxSlots; ++tries) {
        const DemuxSlot slot = d.tab[q];
        if (slot.hash == 0ull) return -1;
        if (slot.hash == h) {
            const uint2 nm = d.name_off[slot.id];
            if (nm.y == n && same_bytes(d.arena + nm.x, p, n)) return (int32_t)slot.id;
        }
        q = (q + 1u) & (kDemuxSlots - 1u);
    }
    return -1;
}

// entry `idx` (2 * line + reading) claims the pending slot of hash h, probing from `start`
__device__ __forceinline__ void demux_claim(const DemuxArgs& d, uint32_t idx, unsigned long long h, uint32_t start) {
    uint32_t q = start & (kDemuxSlots - 1u);
    for (uint32_t tries = 0;; ++tries) {
        if (tries >= kDemuxSlots) {  // (every slot taken by other hashes: far beyond what a block may bring)
            atomicOr(&d.state[0], kDemuxFull);
            d.lsamp[idx] = -1;
            return;
        }
        unsigned long long old = *reinterpret_cast<volatile unsigned long long*>(&d.pend[q].hash);
        if (old == 0ull) old = atomicCAS(&d.pend[q].hash, 0ull, h);
        if (old == 0ull) {
            const uint32_t at = atomicAdd(&d.state[1], 1u);
            if (at >= d.max_new) atomicOr(&d.state[0], kDemuxFull);
            if (at < kDemuxMaxSamples) d.pend_list[at] = q;
            break;
        }
        if (old == h) break;
        q = (q + 1u) & (kDemuxSlots - 1u);
    }
    atomicMax(&d.pend[q].inv, ~idx);
    d.lsamp[idx] = (int32_t)(q | kDemuxAtSlot);
}

// a thread per line; the lines that lead a run look their run's samples up (behind dtok_runs and, where they run,
// dtok_submap / dtok_excl_*: a run whose reads are all dropped brings no sample)
// kEx: behind a scan of the "ex" flavour (coord-match) a reading brings its sample only when it has a hit -- a mapped
// line of aligned length > 0 (ordinal.py:231): ordinal_mapper never yields a read whose hits are all of length 0
template <bool kEx>
__global__ void __launch_bounds__(kDtokThreads) demux_lookup_kernel(DtokArgs a, DemuxArgs d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines) return;
    d.lsamp[2u * i] = -1;
    d.lsamp[2u * i + 1u] = -1;
    if (!a.is_start[i]) return;
    bool need[2] = {false, false};
    uint32_t j = i;
    do {
        if (a.lsubj[j] >= 0 && (!kEx || a.llen[j] > 0u)) need[(a.lmeta[j] >> 28) ? 1 : 0] = true;
        ++j;
    } while (j < a.n_lines && !a.is_start[j]);
    const DemuxName n0 = demux_sample(a, i, 0u), n1 = demux_sample(a, i, 1u);
    if (need[0] && need[1] && n0.len == n1.len) need[1] = false;  // (one name either way)
    for (uint32_t r = 0; r < 2u; ++r) {
        if (!need[r]) continue;
        const DemuxName nm = r ? n1 : n0;
        const unsigned long long h = demux_hash(d, a.text + nm.off, nm.len);
        if (demux_find(d, a.text + nm.off, nm.len, h) >= 0) continue;
        demux_claim(d, 2u * i + r, h, demux_home(h));
    }
}

// a thread per line: the entries that sit in a pending slot compare their bytes with the slot's first claimant's
__global__ void __launch_bounds__(kDtokThreads) demux_verify_kernel(DtokArgs a, DemuxArgs d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines) return;
    for (uint32_t r = 0; r < 2u; ++r) {
        const uint32_t idx = 2u * i + r;
        const int32_t v = d.lsamp[idx];
        if (v < 0 || !((uint32_t)v & kDemuxAtSlot)) continue;
        const uint32_t s = (uint32_t)v & (kDemuxSlots - 1u);
        const uint32_t w = ~d.pend[s].inv;
        bool same = w == idx;
        if (!same) {
            const DemuxName mine = demux_sample(a, i, r), theirs = demux_sample(a, w >> 1, w & 1u);
            same = mine.len == theirs.len && same_bytes(a.text + mine.off, a.text + theirs.off, mine.len);
        }
        if (same) {
            d.lsamp[idx] = -1;
        } else {  // (another name of the same hash: on to the next slot)
            d.lsamp[idx] = (int32_t)((s + 1u) & (kDemuxSlots - 1u));
            atomicAdd(&d.state[2], 1u);
        }
    }
}

// a thread per line: the entries the verification sent on claim again
__global__ void __launch_bounds__(kDtokThreads) demux_reclaim_kernel(DtokArgs a, DemuxArgs d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines) return;
    for (uint32_t r = 0; r < 2u; ++r) {
        const uint32_t idx = 2u * i + r;
        const int32_t v = d.lsamp[idx];
        if (v < 0 || ((uint32_t)v & kDemuxAtSlot)) continue;
        const DemuxName nm = demux_sample(a, i, r);
        demux_claim(d, idx, demux_hash(d, a.text + nm.off, nm.len), (uint32_t)v);
    }
}

// a thread per pending name: (first claimant, offset, length) for the host
__global__ void __launch_bounds__(kDtokThreads) demux_pending_kernel(DtokArgs a, DemuxArgs d, uint32_t n, uint4* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t w = ~d.pend[d.pend_list[t]].inv;
    const DemuxName nm = demux_sample(a, w >> 1, w & 1u);
    out[t] = make_uint4(w, nm.off, nm.len, 0u);
}

// The plain flavour's block as a CSR chunk (the counterpart of dtok_place_kernel): behind dtok_first, dtok_hits<false>
// and the line scan, a thread per first line of a read.  A record's place = records before its run + records of
// lower mates in the run + its position in its read (dtok_place_words_kernel); a read's index likewise from its first
// record, which also looks the read's sample up: its group, and -- unless the whitelist drops it -- the sample's
// "met" byte (a plain store: every writer stores 1).
// `rsamp` (optional): the sample id of every read next to its group, -1 for a read the whitelist drops or whose
// sample the table does not hold (the read maps under demultiplexing cut their text by it, wk_readmap_demux.hpp).
__global__ void __launch_bounds__(kDtokThreads) demux_place_reads_kernel(DtokArgs a, DemuxArgs d, int32_t* __restrict__ rsamp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines || !(a.is_first[i] & 1u)) return;
    const uint32_t m = a.lmeta[i] >> 28;
    uint32_t s = i, before = 0, mine = 0, after = 0, groups_before = 0;
    bool seen[3] = {false, false, false};
    while (!a.is_start[s]) {
        --s;
        if (a.is_first[s] & 1u) {
            const uint32_t q = a.lmeta[s] >> 28;
            before += q < m ? 1u : 0u;
            mine += q == m ? 1u : 0u;
            if (q < 3u) seen[q] = true;
        }
    }
    for (uint32_t j = i + 1u; j < a.n_lines && !a.is_start[j]; ++j)
        if (a.is_first[j] & 1u) {
            const uint32_t q = a.lmeta[j] >> 28;
            before += q < m ? 1u : 0u;
            after += q == m ? 1u : 0u;
            if (q < 3u) seen[q] = true;
        }
    if (mine + 1u + after > (uint32_t)WK_MAX_K) {  // (more candidates than a count key can say: the host evaluates such a read)
        atomicOr(&a.state->flags, kDtokBigRead);
        return;
    }
    const unsigned long long base = a.line_scan[s];  // records / reads before the run
    const uint32_t at = (uint32_t)base + before + mine;
    if (at < d.cap) d.c_subj[at] = a.lsubj[i];
    if (a.is_first[i] & 2u) {  // the read's first record
        for (uint32_t q = 0; q < m && q < 3u; ++q) groups_before += seen[q] ? 1u : 0u;
        const uint32_t r = (uint32_t)(base >> 32) + groups_before;
        const DemuxName nm = demux_sample(a, i, m ? 1u : 0u);
        const int32_t id = demux_find(d, a.text + nm.off, nm.len, demux_hash(d, a.text + nm.off, nm.len));
        int32_t g = -1;
        if (id < 0) {
            atomicOr(&d.state[0], kDemuxMissing);
        } else {
            g = d.group[id];
            if (g >= 0) d.met[id] = 1;
        }
        if (r < d.cap) {
            d.c_qoff[r] = (int32_t)at;
            d.c_group[r] = g;
            if (rsamp) rsamp[r] = g >= 0 ? id : -1;
        }
    }
}

// The "ex" flavour's block as the staged hits of the coord-match with a group per read (the counterpart of
// dtok_place_kernel): behind dtok_hits<true> and the line scan, a thread per hit.  The hits go where dtok_place_kernel
// puts them; a read's first hit also looks the read's sample up: its group (-1: outside the whitelist) and its id in
// the table, for demux_met_hits_kernel -- whether the sample is met is known only once the read has matched a gene.
__global__ void __launch_bounds__(kDtokThreads) demux_place_hits_kernel(DtokArgs a, DemuxArgs d, int32_t* __restrict__ rsamp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines || !(a.is_first[i] & 1u)) return;
    const uint32_t m = a.lmeta[i] >> 28;
    // the run: back to its start, forward to its end
    uint32_t s = i, before = 0, mine = 0, groups_before = 0;
    bool seen[3] = {false, false, false};
    while (!a.is_start[s]) {
        --s;
        if (a.is_first[s] & 1u) {
            const uint32_t q = a.lmeta[s] >> 28;
            before += q < m ? 1u : 0u;
            mine += q == m ? 1u : 0u;
            if (q < 3u) seen[q] = true;
        }
    }
    for (uint32_t j = i + 1u; j < a.n_lines && !a.is_start[j]; ++j)
        if (a.is_first[j] & 1u) {
            const uint32_t q = a.lmeta[j] >> 28;
            before += q < m ? 1u : 0u;
            if (q < 3u) seen[q] = true;
        }
    const unsigned long long base = a.line_scan[s];  // hits / reads before the run
    const uint32_t at = (uint32_t)base + before + mine;
    if (at < d.cap) {
        const int32_t sid = a.lsubj[i];
        a.o_genome[at] = (uint32_t)sid < a.n_gmap ? a.gmap[sid] : -1;
        a.o_beg[at] = a.lbeg[i];
        a.o_end[at] = a.lend[i];
        a.o_len[at] = a.llen[i];
    }
    if (a.is_first[i] & 2u) {  // the read's first hit: its offset, its sample
        for (uint32_t q = 0; q < m && q < 3u; ++q) groups_before += seen[q] ? 1u : 0u;
        const uint32_t r = (uint32_t)(base >> 32) + groups_before;
        const DemuxName nm = demux_sample(a, i, m ? 1u : 0u);
        const int32_t id = demux_find(d, a.text + nm.off, nm.len, demux_hash(d, a.text + nm.off, nm.len));
        if (id < 0) atomicOr(&d.state[0], kDemuxMissing);
        if (r < d.cap) {
            a.o_hoff[r] = (int32_t)at;
            d.c_group[r] = id < 0 ? -1 : d.group[id];
            rsamp[r] = id;
        }
    }
}

// behind wk_ordinal_match, a thread per read: a read that matched a gene and whose sample the whitelist keeps makes
// its sample one the reference has met (a plain store: every writer stores 1)
__global__ void __launch_bounds__(kDtokThreads) demux_met_hits_kernel(const int32_t* __restrict__ qoff, const int32_t* __restrict__ group,
                                                                      const int32_t* __restrict__ rsamp, int64_t n_reads, uint32_t n_samples,
                                                                      unsigned char* __restrict__ met) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    if (qoff[r + 1] > qoff[r] && group[r] >= 0) {
        const int32_t id = rsamp[r];
        if ((uint32_t)id < n_samples) met[id] = 1;
    }
}

}  // namespace wk
