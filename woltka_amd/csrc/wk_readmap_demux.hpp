// wk_readmap_demux.hpp — the read maps of `--outmap` under demultiplexing, formatted on the device.
//
// Under `--demux` (and for every single-file input) workflow.demultiplex (workflow.py:886-907) cuts a read id --
// QNAME plus "/1" | "/2" for a mate -- at its first '_': `sample = right and left`, `read = right or left`.  Per
// chunk and sample file.write_readmap appends to `<dir>/<sample>.txt`, so a sample's file holds its reads in file
// order, each line formatted on its own and headed by the *read* part of the id:
//
//   no '_' in the id                  sample '',   read = the whole id
//   "S1_"  unpaired                   sample '',   read = "S1" (the '_' is gone)
//   "S1_"  as a mate ("S1_/1")        sample "S1", read = "/1"
//   otherwise                         read = everything behind the first '_', mate suffix included
//
// (readmap_id<true>, wk_readmap_reads.hpp; demux_sample, wk_demux.hpp, is the sample side of the same rule.)
//
// The block is the staged chunk of wk_dtok_stage_reads_samples: wk_dtok_stage_reads' chunk with the sample id of
// every read kept next to its group (demux_place_reads_kernel, `rsamp`: -1 for a read the whitelist drops) and the
// reads' leader lines (readmap_leaders_kernel).  Per job the lines' lengths come from the demux variants of the
// two formatters' length steps, their places from the partition below, and the demux variants of the write steps
// put every line where the partition said: the text of the block is one run per sample, samples ascending by id,
// each run in read order.  The host appends every run to its sample's file.
//
// The partition (readmap_demux_*): from samp[n] (-1: no line) and len[n] (0: no line)
//   off[r]   = the sum of len over all (samp', r') < (samp, r), lexicographically: a stable partition by sample,
//   segments = (sample id, first byte, bytes) of the samples present, ascending by id,
//   total    = all bytes.
// Separate launches, integer sums in a fixed order, no workgroup waits for another:
//   mark     a thread per read: present[samp] = 1                       (every writer stores 1)
//   rank     one workgroup: the exclusive scan of present[0, 65 536): a sample's column d, their number D
//   tile     a workgroup per tile of kPartTile reads: a read's bytes before it in its tile and sample (each thread
//            walks the tile's (column, length) pairs in LDS), the tile's bytes per sample -> mat[tile][d]
//   columns  down the columns of mat: a workgroup per 64 columns, 16 strips of tiles each summed, then rescanned
//            from the strips' bases; the columns' totals
//   across   one workgroup: the exclusive scan of the columns' totals, the segment table, the total
//   add      a thread per read: off = column base + tiles above + within the tile
//
// Limits: tiles x D entries of `mat` -- the caller refuses a block beyond the capacity it has reserved
// (option "readmap_demux_cap") before anything is written; sample ids below kDemuxMaxSamples.
#pragma once
#include "wk_demux.hpp"
#include "wk_readmap_lists.hpp"

namespace wk {

constexpr uint32_t kPartTile = 512;       // reads of a tile (WK_READMAP_DEMUX_TILE)
constexpr uint32_t kPartNone = 0xFFFFFFFFu;
constexpr uint32_t kPartScanThreads = 1024;
constexpr uint32_t kPartPerThread = kDemuxMaxSamples / kPartScanThreads;  // 64 ids a thread
constexpr uint32_t kPartStrips = 16;
// entries of the matrix (tiles x samples of a block): the default takes a 64 MB block -- 1.6 M reads at most, 3200
// tiles -- at 2600 samples in 64 MB; the most an option may ask for is 2 GB
constexpr int64_t kPartCapDefault = 1ll << 23, kPartCapMax = 1ll << 28;
static_assert(kPartTile == WK_READMAP_DEMUX_TILE, "the header names the tile");
static_assert(kDemuxMaxSamples % kPartScanThreads == 0, "the id scan gives every thread the same share");

// ---- the formatters' demux variants ------------------------------------------------------------------------------

// a thread per read: the length of its line (0 for a read the whitelist drops)
__global__ void __launch_bounds__(kDtokThreads) readmap_reads_len_demux_kernel(DtokArgs a, ReadmapReadsArgs m, const int32_t* __restrict__ samp) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m.n_reads) return;
    m.read_len[r] = samp[r] < 0 ? 0ull : readmap_reads_line_len<true>(a, m, r, m.assign[r]);
}

// a thread per read: its line at read_len[r] (the place the partition gave it)
__global__ void __launch_bounds__(kDtokThreads) readmap_reads_write_demux_kernel(DtokArgs a, ReadmapReadsArgs m, const int32_t* __restrict__ samp) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m.n_reads || samp[r] < 0) return;
    readmap_reads_write_line<true>(a, m, r, m.assign[r]);
}

__global__ void __launch_bounds__(kDtokThreads) readmap_lists_build_demux_kernel(DtokArgs a, ReadmapListsArgs L, const int32_t* __restrict__ samp) {
    lists_build_tile<true>(a, L, samp);
}

__global__ void __launch_bounds__(kDtokThreads) readmap_lists_write_demux_kernel(DtokArgs a, ReadmapListsArgs L, const int32_t* __restrict__ samp) {
    lists_write_tile<true>(a, L, samp);
}

// ---- the partition -----------------------------------------------------------------------------------------------

struct PartArgs {
    const int32_t* samp;              // [n]
    const unsigned long long* len;    // [n]
    unsigned long long* off;          // [n]
    uint32_t* present;                // [kDemuxMaxSamples] 0 | 1 -> (rank) the sample's column
    uint32_t* n_cols;                 // [1] D
    unsigned long long* mat;          // [tiles x D]
    unsigned long long* col;          // [D] bytes of a column -> its first byte
    unsigned long long* seg;          // [3 x kDemuxMaxSamples] (sample id, first byte, bytes) of the D columns
    unsigned long long* total;        // [1]
    uint32_t* flags;                  // [1] 1: a sample id outside the table
    uint32_t n;
    uint32_t n_tiles;
};

// a thread per read
__global__ void __launch_bounds__(kDtokThreads) readmap_demux_mark_kernel(PartArgs p) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n) return;
    const int32_t s = p.samp[r];
    if (s < 0) return;
    if ((uint32_t)s < kDemuxMaxSamples)
        p.present[s] = 1u;
    else
        atomicOr(p.flags, 1u);
}

// Exclusive scan of v[0, kDemuxMaxSamples) by one workgroup of kPartScanThreads threads, kPartPerThread consecutive
// entries a thread: returns the prefix in front of this thread's entries, *all = the sum.
template <typename T>
__device__ __forceinline__ T part_scan_base(T mine, T* lds, T* all) {
    const uint32_t tid = threadIdx.x;
    lds[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < kPartScanThreads; d <<= 1) {
        const T u = tid >= d ? lds[tid - d] : (T)0;
        __syncthreads();
        lds[tid] += u;
        __syncthreads();
    }
    *all = lds[kPartScanThreads - 1];
    return lds[tid] - mine;
}

// one workgroup: present[s] (0 | 1) -> the column of sample s (kPartNone: absent), seg[3 d] = s, *n_cols = D
__global__ void __launch_bounds__(kPartScanThreads) readmap_demux_rank_kernel(PartArgs p) {
    __shared__ uint32_t lds[kPartScanThreads];
    const uint32_t first = threadIdx.x * kPartPerThread;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < kPartPerThread; ++k) mine += p.present[first + k] ? 1u : 0u;
    uint32_t all;
    uint32_t d = part_scan_base<uint32_t>(mine, lds, &all);
    for (uint32_t k = 0; k < kPartPerThread; ++k) {
        const bool here = p.present[first + k] != 0u;
        p.present[first + k] = here ? d : kPartNone;
        if (here) p.seg[3u * d] = first + k;
        d += here ? 1u : 0u;
    }
    if (threadIdx.x == 0) *p.n_cols = all;
}

// a workgroup per tile of kPartTile reads (mat is zero: an entry is written only where the tile holds the sample)
__global__ void __launch_bounds__(kPartTile) readmap_demux_tile_kernel(PartArgs p, uint32_t n_cols) {
    __shared__ uint32_t col_s[kPartTile];
    __shared__ unsigned long long len_s[kPartTile];
    const uint32_t tid = threadIdx.x;
    const uint32_t r = blockIdx.x * kPartTile + tid;
    uint32_t d = kPartNone;
    unsigned long long len = 0;
    if (r < p.n) {
        const int32_t s = p.samp[r];
        if (s >= 0 && (uint32_t)s < kDemuxMaxSamples) {
            d = p.present[s];
            len = p.len[r];
        }
    }
    if (d >= n_cols) d = kPartNone;  // (a column the matrix does not have)
    col_s[tid] = d;
    len_s[tid] = len;
    __syncthreads();
    if (d == kPartNone) {
        if (r < p.n) p.off[r] = 0ull;
        return;
    }
    unsigned long long before = 0;
    bool last = true;
    for (uint32_t j = 0; j < kPartTile; ++j)
        if (col_s[j] == d) {
            if (j < tid)
                before += len_s[j];
            else if (j > tid)
                last = false;
        }
    p.off[r] = before;
    if (last && blockIdx.x < p.n_tiles) p.mat[(size_t)blockIdx.x * n_cols + d] = before + len;
}

// a workgroup per 64 columns: thread (x = column, y = strip of tiles)
__global__ void __launch_bounds__(kWave * kPartStrips) readmap_demux_columns_kernel(PartArgs p, uint32_t n_cols) {
    __shared__ unsigned long long strip[kPartStrips][kWave];
    const uint32_t x = threadIdx.x & (kWave - 1), y = threadIdx.x / kWave;
    const uint32_t d = blockIdx.x * kWave + x;
    const uint32_t per = (p.n_tiles + kPartStrips - 1) / kPartStrips;
    const uint32_t t0 = y * per < p.n_tiles ? y * per : p.n_tiles;
    const uint32_t t1 = t0 + per < p.n_tiles ? t0 + per : p.n_tiles;
    unsigned long long sum = 0;
    if (d < n_cols)
        for (uint32_t t = t0; t < t1; ++t) sum += p.mat[(size_t)t * n_cols + d];
    strip[y][x] = sum;
    __syncthreads();
    if (d >= n_cols) return;
    unsigned long long base = 0, all = 0;
    for (uint32_t k = 0; k < kPartStrips; ++k) {
        const unsigned long long v = strip[k][x];
        if (k < y) base += v;
        all += v;
    }
    for (uint32_t t = t0; t < t1; ++t) {
        const size_t at = (size_t)t * n_cols + d;
        const unsigned long long v = p.mat[at];
        p.mat[at] = base;
        base += v;
    }
    if (y == 0) p.col[d] = all;
}

// one workgroup: col[d] (bytes) -> the column's first byte; the segment table; the total
__global__ void __launch_bounds__(kPartScanThreads) readmap_demux_across_kernel(PartArgs p, uint32_t n_cols) {
    __shared__ unsigned long long lds[kPartScanThreads];
    const uint32_t first = threadIdx.x * kPartPerThread;
    unsigned long long mine = 0;
    for (uint32_t k = 0; k < kPartPerThread; ++k)
        if (first + k < n_cols) mine += p.col[first + k];
    unsigned long long all;
    unsigned long long at = part_scan_base<unsigned long long>(mine, lds, &all);
    for (uint32_t k = 0; k < kPartPerThread; ++k) {
        const uint32_t d = first + k;
        if (d >= n_cols) break;
        const unsigned long long bytes = p.col[d];
        p.col[d] = at;
        p.seg[3u * d + 1u] = at;
        p.seg[3u * d + 2u] = bytes;
        at += bytes;
    }
    if (threadIdx.x == 0) *p.total = all;
}

// a thread per read
__global__ void __launch_bounds__(kDtokThreads) readmap_demux_add_kernel(PartArgs p, uint32_t n_cols) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n) return;
    const int32_t s = p.samp[r];
    if (s < 0 || (uint32_t)s >= kDemuxMaxSamples) return;
    const uint32_t d = p.present[s];
    if (d >= n_cols) return;
    p.off[r] += p.col[d] + p.mat[(size_t)(r / kPartTile) * n_cols + d];
}

}  // namespace wk
