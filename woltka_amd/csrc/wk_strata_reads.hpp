// wk_strata_reads.hpp — plain classification with `--stratify` on the device text route.
//
// classify.counter_strat (woltka/classify.py:216-249) counts a query under the stratum its
// read id has in the sample's map and skips the queries the map does not hold.  The map is
// the join table of wk_strata.hpp; here a block the device tokenizer has scanned for the
// plain flavour (wk_dtok.hpp) becomes the CSR chunk the general evaluator counts
// (wk_classify.hpp) with a group per read -- the (sample, stratum) group of its label, or -1
// for a read the map does not hold -- the way demux_place_reads_kernel (wk_demux.hpp) does
// it for the samples of `--demux`.
//
// Limits: a read of more than WK_MAX_K candidates sets kDtokBigRead and the host tokenizer
// takes the block.
#pragma once
#include "wk_dtok.hpp"
#include "wk_strata.hpp"

namespace wk {

struct StrataChunk {
    int32_t* c_subj;   // [cap] subjects, read by read
    int32_t* c_qoff;   // [cap] first record of every read
    int32_t* c_group;  // [cap] group of every read, -1: not counted
    uint32_t cap;      // records / reads the arrays hold
};

// Behind dtok_first, dtok_hits<false> and the line scan, a thread per first line of a (read, subject).  A record's
// place = records before its run + records of lower mates in the run + its position in its read; a read's index
// likewise from its first record (the places demux_place_reads_kernel computes).  The read's first record alone looks
// its id up: QNAME (+ "/1" | "/2" for a mate) as the per-line arrays of the plain flavour have it.
// kJoin = false: no map, no group per read (the caller names one group for the chunk): the places alone.
template <bool kJoin>
__global__ void __launch_bounds__(kDtokThreads) strata_place_reads_kernel(DtokArgs a, StrataArgs strata, StrataChunk ch) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines || !(a.is_first[i] & 1u)) return;
    const uint32_t m = a.lmeta[i] >> 28;
    uint32_t s = i, before = 0, mine = 0, after = 0, groups_before = 0;
    bool seen[3] = {false, false, false};
    while (!a.is_start[s]) {  // (a mapped line in front of i starts the run: s never passes 0)
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
    if (at < ch.cap) ch.c_subj[at] = a.lsubj[i];
    if (a.is_first[i] & 2u) {  // the read's first record
        for (uint32_t q = 0; q < m && q < 3u; ++q) groups_before += seen[q] ? 1u : 0u;
        const uint32_t r = (uint32_t)(base >> 32) + groups_before;
        int32_t g = 0;
        if constexpr (kJoin) g = strata_lookup(strata, a.text + a.line_start[i], a.lmeta[i] & 0x0FFFFFFFu, m);
        if (r < ch.cap) {
            ch.c_qoff[r] = (int32_t)at;
            ch.c_group[r] = g;
        }
    }
}

}  // namespace wk
