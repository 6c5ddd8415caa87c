// wk_readmap_reads.hpp — the read maps of `--outmap` for whole-read assignments, formatted on the device.
//
// Under `--rank free`, and under a rank (or none) with --uniq / --above / --major, a read's result is one
// feature or nothing (classify.assign_free, classify.assign_rank, classify.assign_none with uniq;
// classify.py:32-141): file.write_readmap (file.py:469-500) prints `query[/mate] <tab> feature` for it, and
// `Unassigned` for a read without one under --unassigned (workflow.py:1038-1039).  The block is the staged
// classify chunk of wk_dtok_stage_reads_plain (stage_reads_chunk), whose reads stand in the order
// align.py:327-332 yields them; classify_kernel has left a code per (job, read) in the device's assignment
// buffer (wk_classify_staged_keep).  The line of a read is built from that code, the QNAME at the read's
// leader line and the shown-text table -- feature id -> the bytes printed: the id, or its name under
// --name-as-id -- which covers the hierarchy's nodes and the names outside it (ids >= n_nodes: subjects that
// are no node, met under `--rank none --uniq` and --subok).
//
// Kernels: readmap_leaders (a thread per line: the leader line of every read, once per block), then per
// job readmap_reads_len (a thread per read), the scan of the lengths (u64_tile_*, wk_readmap.hpp) and
// readmap_reads_write (a thread per read).
//
// Limits: a code that says "a list" or "no candidates" (WK_ASSIGN_MULTI / WK_ASSIGN_EMPTY: the job sets of
// this route cannot give one) or a feature outside the table raises kReadsBadCode; no line is written for it.
#pragma once
#include "wk_readmap.hpp"

namespace wk {

constexpr uint32_t kReadsBadCode = 1u;

struct ReadmapReadsArgs {
    const int32_t* assign;           // [n_reads] codes of the job: feature id or WK_ASSIGN_*
    const uint32_t* read_line;       // [n_reads] leader line of the read
    const uint32_t* shown_off;       // [n_shown + 1]
    const unsigned char* shown;      // text printed per feature
    uint32_t n_shown;
    unsigned long long* read_len;    // [n_reads] length of its map line -> exclusive prefix
    uint32_t* flags;                 // kReadsBadCode
    unsigned char* out;
    unsigned long long out_cap;
    uint32_t n_reads;
    uint32_t unassigned;             // --unassigned: a read without a feature is printed as such
};

__device__ const unsigned char kUnassignedText[10] = {'U', 'n', 'a', 's', 's', 'i', 'g', 'n', 'e', 'd'};

// a thread per line; leaders tell their read where its QNAME is
__global__ void __launch_bounds__(kDtokThreads) readmap_leaders_kernel(DtokArgs a, uint32_t* __restrict__ read_line, uint32_t n_reads) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_lines || !(a.is_first[i] & 2u)) return;
    const uint32_t r = readmap_read_index(a, i);
    if (r < n_reads) read_line[r] = i;
}

// The bytes of the id of the read led by line i that a map line prints in front of the mate suffix: (offset in
// the text, length).  kDemux: the read part of the id as workflow.demultiplex leaves it (wk_readmap_demux.hpp).
struct ReadmapId {
    uint32_t off, n;
    bool mate;  // "/1" | "/2" follows
};

template <bool kDemux>
__device__ __forceinline__ ReadmapId readmap_id(const DtokArgs& a, uint32_t i) {
    const uint32_t lo = a.line_start[i], meta = a.lmeta[i];
    const uint32_t qn = meta & 0x0FFFFFFFu;
    const bool mate = (meta >> 28) != 0u;
    if (!kDemux) return ReadmapId{lo, qn, mate};
    uint32_t u = qn;
    for (uint32_t k = 0; k < qn; ++k)
        if (a.text[lo + k] == '_') {
            u = k;
            break;
        }
    if (u == qn) return ReadmapId{lo, qn, mate};                    // no '_': the whole id
    if (u + 1u == qn && !mate) return ReadmapId{lo, qn - 1u, false};  // "S1_" unpaired: right is empty, the read is left
    return ReadmapId{lo + u + 1u, qn - u - 1u, mate};                 // everything behind the first '_'
}

// Bytes shown for code v: 0 = no line.  A code that cannot be printed raises the flag.
__device__ __forceinline__ uint32_t readmap_reads_shown(const ReadmapReadsArgs& m, int32_t v) {
    if (v >= 0) {
        if ((uint32_t)v >= m.n_shown) {
            atomicOr(m.flags, kReadsBadCode);
            return 0u;
        }
        return m.shown_off[v + 1] - m.shown_off[v];
    }
    if (v == WK_ASSIGN_NONE) return m.unassigned ? (uint32_t)sizeof kUnassignedText : 0u;
    atomicOr(m.flags, kReadsBadCode);
    return 0u;
}

// The length of read r's line under code v (0: none)
template <bool kDemux = false>
__device__ __forceinline__ unsigned long long readmap_reads_line_len(const DtokArgs& a, const ReadmapReadsArgs& m, uint32_t r, int32_t v) {
    const uint32_t i = m.read_line[r];
    unsigned long long len = 0;
    // (a feature with an empty id still has its line: only "nothing" has none)
    const uint32_t shown = readmap_reads_shown(m, v);
    const bool line = i < a.n_lines && ((v >= 0 && (uint32_t)v < m.n_shown) || (v == WK_ASSIGN_NONE && m.unassigned));
    if (line) {
        const ReadmapId id = readmap_id<kDemux>(a, i);
        len = (unsigned long long)id.n + (id.mate ? 2u : 0u) + 1u + shown + 1u;
    }
    return len;
}

// a thread per read: the length of its line
__global__ void __launch_bounds__(kDtokThreads) readmap_reads_len_kernel(DtokArgs a, ReadmapReadsArgs m) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m.n_reads) return;
    m.read_len[r] = readmap_reads_line_len(a, m, r, m.assign[r]);
}

// Read r's line under code v at read_len[r] (now the exclusive prefix, or the place the partition gave it)
template <bool kDemux = false>
__device__ __forceinline__ void readmap_reads_write_line(const DtokArgs& a, const ReadmapReadsArgs& m, uint32_t r, int32_t v) {
    const uint32_t i = m.read_line[r];
    if (i >= a.n_lines) return;
    const unsigned char* s;
    uint32_t n;
    if (v >= 0 && (uint32_t)v < m.n_shown) {
        s = m.shown + m.shown_off[v];
        n = m.shown_off[v + 1] - m.shown_off[v];
    } else if (v == WK_ASSIGN_NONE && m.unassigned) {
        s = kUnassignedText;
        n = (uint32_t)sizeof kUnassignedText;
    } else {
        return;
    }
    unsigned long long at = m.read_len[r];
    const ReadmapId id = readmap_id<kDemux>(a, i);
    const uint32_t qn = id.n, mate = id.mate ? a.lmeta[i] >> 28 : 0u;
    if (at + qn + (mate ? 2u : 0u) + 2u + n > m.out_cap) return;  // (the lengths said otherwise: nothing past the text)
    unsigned char* o = m.out;
    const unsigned char* q = a.text + id.off;
    for (uint32_t k = 0; k < qn; ++k) o[at + k] = q[k];
    at += qn;
    if (mate) {
        o[at++] = '/';
        o[at++] = (unsigned char)('0' + mate);
    }
    o[at++] = '\t';
    for (uint32_t k = 0; k < n; ++k) o[at + k] = s[k];
    at += n;
    o[at] = '\n';
}

// a thread per read: its line
__global__ void __launch_bounds__(kDtokThreads) readmap_reads_write_kernel(DtokArgs a, ReadmapReadsArgs m) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m.n_reads) return;
    readmap_reads_write_line(a, m, r, m.assign[r]);
}

}  // namespace wk
