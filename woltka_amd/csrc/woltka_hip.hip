// woltka_hip.hip — C-ABI implementation of include/woltka_hip.h for gfx950.
// Host-side resource management + kernel launches.  No CPU compute path: every
// entry point that does work launches HIP kernels on the context's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <ctime>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/woltka_hip.h"
#include "../../include/woltka_hip_measure.h"
#include "wk_classify.hpp"
#include "wk_cover.hpp"
#include "wk_device.hpp"
#include "wk_dtok.hpp"
#include "wk_demux.hpp"
#include "wk_strata_reads.hpp"
#include "wk_dtok_fused.hpp"
#include "wk_free.hpp"
#include "wk_ordinal.hpp"
#include "wk_stripe.hpp"
#include "wk_readmap.hpp"
#include "wk_readmap_reads.hpp"
#include "wk_readmap_lists.hpp"
#include "wk_readmap_demux.hpp"
#include "wk_tok_internal.h"
#include "wk_weigh.hpp"
#include "wk_weigh_wide.hpp"
#include "wk_sized.hpp"
#include "wk_logred.hpp"
#include "wk_dinflate.hpp"

using namespace wk;

namespace {

thread_local std::string g_last_error;  // for calls without a context

// growable device buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return e;
        }
        size_t want = bytes + bytes / 4 + 256;  // headroom against re-allocation churn
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, bytes);
            want = bytes;
            if (e != hipSuccess) {
                p = nullptr;
                return e;
            }
        }
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// Kernel timing (wk_profile_kernels): the timed launches of one API call form a
// chain of events — one at the call's start, one behind every timed family — and
// a family's time runs from the event before it to its own.  The brackets of a
// call therefore add up to the call's time on the stream (a pair of events of
// its own around every small kernel read 30 us for 10 us kernels).
struct KernelTimer {
    hipEvent_t b = nullptr;     // behind the family's launches
    hipEvent_t from = nullptr;  // the chain's event before them (not owned)
    bool valid = false;
};

// One buffer of block text on the device (wk_ctx::text_buf) and what belongs to the block it holds.  A buffer is free,
// holds a block copied ahead (tagged by `src` / `n`), is the one the kernels of the block scanned last read (until
// the next scan begins), or is read by a block whose verdict is still out (wk_dtok_scan_emit_begin).  wk_dtok_copy
// may be called from another thread than the scans (the host layer's reader thread issues the copies as soon as a
// block is cut): `state` and the tag -- `src`, `n`, `seq` -- are guarded by wk_ctx::copy_mu.  `counted`, `detached` and
// `last` describe the tagged block: written before the tag is, read once it has been found.  The rest belongs to
// whoever holds the buffer by its state.
struct TextBuf {
    unsigned char state = 0;       // wk_ctx::kBufFree ...
    const char* src = nullptr;     // the tag: host address and length of the block
    uint32_t n = 0;
    unsigned long long seq = 0;    // blocks are scanned in the order they were copied: a copy's number tells two buffers with the same tag apart
    bool counted = false;          // the block's newlines were counted behind its copy (`tiles`, `tile_off`, wk_ctx::copy_newlines[k])
    // a block copied by wk_dtok_copy_ahead: the host bytes are not kept until the scan (the reader reuses its pinned
    // buffer once the copy is through); what the scan wants from them comes back from the device when it does
    bool detached = false;
    char last = 0;                 // the block's last byte (a last line without newline)
    hipEvent_t ev0 = nullptr;      // start of the block's copy
    hipEvent_t evm = nullptr;      // ... its end (the newline count behind it runs on a stream of its own)
    hipEvent_t ev = nullptr;       // ... and the end of that count
    unsigned char* text = nullptr; // the device memory: a share of a slab, or `own` (text_buffer())
    DevBuf own;
    DevBuf tiles, tile_off;        // newlines per tile of a block copied ahead, counted behind its copy
    // a block wk_dtok_inflate_ahead fills: compressed bytes, members' spans and status words (wk_dinflate.hpp); the
    // kernel's "a member failed" word lands in wk_ctx::di_any_host[k] (read by wk_dtok_copy_wait)
    DevBuf di_comp, di_meta, di_status;
    bool di_used = false;
    std::vector<int64_t> di_meta_host;   // what the copies of the block's spans and carry read until they are through
    std::vector<char> di_carry_host;
};

}  // namespace

struct wk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    hipDeviceProp_t prop;

    // hierarchy
    DevBuf nodes, rank_code;
    int32_t n_nodes = 0;
    DevBuf rank_tab[WK_MAX_JOBS * 4];
    bool rank_tab_valid[WK_MAX_JOBS * 4] = {};
    int32_t rank_tab_code[WK_MAX_JOBS * 4] = {};
    int64_t rank_tab_nodes[WK_MAX_JOBS * 4] = {};  // nodes that carry the slot's rank (distinct results a job can have)
    std::vector<int32_t> rank_code_host;           // host copy of the rank codes (for those counts)
    // host copies of the tree and the subject table + what `--rank free` looks up
    // instead of walking (ClassifyArgs::free_sparse): subjects ranked by pre-order
    // id, LCAs of rank-adjacent subjects as a sparse table; rebuilt when either changes
    std::vector<int32_t> parent_host, last_host, subj_feat_host;
    int tree_serial = 0, subj_serial = 0, free_tree = -1, free_subj = -1;
    DevBuf f_rank, f_sparse;
    // tables of the per-read stream (wk_free.hpp) for one job: over the nodes its
    // records can name — the subjects' nodes (kind 1, `--rank free`) or their
    // ancestors at the job's rank (kind 2)
    struct StreamTables {
        DevBuf dsparse, dparent, dself, rnode;
        // the distinct nodes the stream's records can name, ascending — a record names one by its index — and per
        // subject that index (-1: the subject has no node); what they were made for
        std::vector<int32_t> dn_host;
        DevBuf subj_rank;
        int rk_kind = -1, rk_slot = -1, rk_tree = -1, rk_subj = -1, rk_rank = -1;
        DevBuf subj_node;                    // kind 2: ancestor at the rank per subject (-1: none)
        std::vector<int32_t> subj_node_host;
        int node_slot = -1, node_tree = -1, node_rank = -1;  // what subj_node_host was made for
        uint32_t dm = 0, results = 0;
        int kind = -1, slot = -1, tree = -1, subj = -1, rank = -1;  // what the tables were made for
    };
    StreamTables st[WK_MAX_JOBS];
    DevBuf w_tmp;  // (unused since the stream translates subject indices itself: free_stream_kernel<., true>)
    DevBuf w_renum;  // old rank -> new rank when the subject table grows under accumulated records
    DevBuf f_dense;  // reads per result node of the free-rank stream
    DevBuf f_log, f_log_cnt, f_partial, f_part_used;  // results the stream's LDS caches had no room for, per wave; their counts per share (free_log_kernel)
    int f_dense_tree = -1;
    uint32_t f_m = 0;
    int use_free_sparse = 1;
    int log_parts_opt = 0;                         // 0 = auto, else 256 / 1024

    // compact subject table (optional)
    DevBuf subj_feat, subj_rows, dense_slab, plog, plog_cnt;
    int use_plog = 1;                     // partitioned miss log (auto: large chunks without dense bins)
    int64_t plog_max_bytes = 4ll << 30;   // upper bound of the miss-log buffer
    int32_t n_subjects = 0;
    int32_t max_subject_feature = -1;
    int use_dense = 1;
    int32_t rows_w = 0;
    std::vector<int> rows_sig;  // rank slots the rows were built for (+ n_subjects)
    bool subj_indexed = false;  // staged chunk carries subject indices

    // genes
    DevBuf gene4, g_grid, g_first, g_goff, g_shift;  // gene tables (wk_set_genes; wk_ordinal.hpp)
    bool genes_set = false;
    bool genes_by_index = false;   // gene lists carry gene table indices (wk_ordinal_pair_genes), translated to features for the classification
    int gene_index_opt = 0;        // asked for by the next wk_set_genes (option "gene_index_pairs")
    DevBuf g_feature, o_pairs_feat;
    int grid_density = 2;  // grid cells per gene (rounded up to a power of two per genome)
    int32_t n_genomes = 0, n_genes = 0;

    // count table
    DevBuf tkeys, tvals;
    uint64_t slots = 0;

    // staged classify chunk
    DevBuf c_subj, c_qoff, c_group;
    const int32_t* cur_subj = nullptr;  // points into c_subj or o_pairs
    const int32_t* cur_qoff = nullptr;
    int64_t n_reads = 0, n_records = 0;
    bool has_group = false, subj_is_set = false, chunk_valid = false;
    int32_t group_base = 0;  // group of every read of a chunk staged without a group array

    // staged ordinal chunk
    DevBuf o_genome, o_beg, o_end, o_len, o_hoff, o_cnt, o_ub, o_first2, o_poff, o_pairs, o_qoff, o_tile_sum, o_tile_off;
    int64_t n_hits = 0, o_reads = 0;
    double th = 0.8;
    bool ord_valid = false;
    // hits binned by genome stripe (wk_stripe.hpp): the stripes of the gene tables, the sorted chunk
    DevBuf g_gene_off, g_stripe_of, g_stripes;
    std::vector<StripeInfo> stripes_host;
    bool stripes_usable = false;
    int use_fused = 1;         // (0: every block through the six kernels of wk_dtok.hpp; wk_tune "dtok_fused")
    uint32_t fused_ablate = 0; // (measurement, wk_tune "fz_ablate")
    std::atomic<bool> fused_streak{false}; // the block scanned last went through the one kernel: copies are not followed by a newline count
    double dt_lpb = 0.0;       // lines per byte of that block
    int fused_per_cu = 3;      // persistent workgroups per CU of dtok_fused_kernel (wk_tune "dtok_fused_per_cu")
    int64_t fused_blocks = 0, fused_fallbacks = 0;   // blocks the fused kernel did / handed back
    hipEvent_t res_ev = nullptr;
    int use_stripes = 1;       // (0: the gather kernels of wk_ordinal.hpp for every read; measurement)
    int64_t chunks_sorted = 0, chunks_gathered = 0;   // (measurement: wk_ordinal_chunk_counts)
    bool acc_open = false;     // the staged hits are blocks piled up by wk_dtok_stage_hits_append, not counted yet
    int64_t stripes_min_hits = 4000000;  // chunks below this keep the gather kernels (wk_tune "stripes_min")
    DevBuf sb_cnt, sb_tot, sb_base, sb_binned, sb_units, sb_over, sb_stat;
    DevBuf r_genome, r_beg, r_end, r_len, r_hoff;
    bool sb_valid = false;     // the staged chunk has been sorted
    int64_t sb_single = 0, sb_rest_reads = 0, sb_rest_hits = 0;
    uint32_t sb_n_units = 0;

    // misc device scalars: [0]=err(int) [3]=total pairs [4]=compact counter [5]=log cursor
    DevBuf scalars;
    DevBuf stat_block;  // kStatBlocks x (reads, records), see flush_stats()
    DevBuf log;         // contribution log of WK_F_SIZED jobs, cursor = scalars[5]
    int64_t log_cap = 0;
    DevBuf assign_out, fetch_k, fetch_v;
    int64_t stat_pairs = 0;

    // timing
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool timer_closed = false;
    bool profile = false;
    std::map<std::string, KernelTimer> ktimers;
    hipEvent_t kt_step = nullptr;   // recorded where a timed API call starts
    hipEvent_t kt_tail = nullptr;   // last event of the chain
    int kt_depth = 0;
    double lap_s[4] = {0, 0, 0, 0};   // (wk_tune "lap_print") seconds inside wk_dtok_copy / scan / waits of scan / emit
    double lap_x[6] = {0, 0, 0, 0, 0, 0};  // ... of the scan: until the buffer is claimed / line starts queued / parse queued / emission queued / finish / names
    double lap_c[5] = {0, 0, 0, 0, 0};  // ... of the copy: streams + events / device buffer / copy queued / count queued; [4] the longest device-buffer step
    double lap_copy_ms = 0;           // ... and the copies' own durations (events around each on the copy stream)
    int64_t lap_copy_bytes = 0;

    int lds_slots = 8192;  // LDS front-cache slots per workgroup (16 B each = 128 KiB)
    int threads = 1024;    // workgroup size of the direct classify kernel
    int use_lds = 1;
    int blocks_per_cu = 1;
    int ablate = 0;  // honoured only by -DWK_ABLATE measurement builds
    int tiled = 0;  // LDS-staged classify kernel (0: direct one-thread-per-read kernel)
    // two-class split (single-candidate pass, then the generic pass over the
    // rest): 0 = off, 1/2 = on whenever the chunk qualifies
    int use_split = 1;
    int single_blocks_per_cu = 1;
    int use_count_kernel = 1;  // count-first pass as count_subjects_kernel (statically pipelined)
    DevBuf left_mask, left_list, first_slab;
    // weighted subject histogram (wk_weigh.hpp): 0 = off, 1 = auto, 2 = whenever applicable
    int use_weigh = 1;
    int tally_per_cu = 3;    // tally workgroups (512 threads) per CU
    int tally_slots = 1024;  // hash-cache slots of a tally workgroup (a power of two)
    int use_tally = 1;      // wk_ordinal_count: genes tallied per read straight from the matches
    int match_lds = 1;      // per-genome words of the coordinate grid in LDS when they fit
    bool listed_only = false;  // wk_classify_staged evaluates only the reads of left_mask
    int bins_ring = 4;  // measurement knob: load stages in flight of weigh_bins_kernel
    DevBuf w_slab, w_hi, w_invalid;
    // the wide layout (wk_weigh_wide.hpp): the records by bucket; the plan, the buckets' counts and their cursors
    DevBuf w_wide, w_wide_plan;
    int weigh_wide = 0;      // measurement knob: 1 = a fresh accumulation opens unsliced and its flush takes the wide layout
    int weigh_wide_wgs = 0;  // measurement knob: workgroups of the wide histogram, at most (0: one per CU)
    size_t w_hi_clean = 0;        // leading entries of w_hi known to be zero
    // size-normalised plain jobs (wk_sized.hpp): rows {feature, subject feature, job << 16 | divisor, group} and their
    // counts, appended by every flush of such a job set until wk_sized_fetch takes them
    DevBuf sz_rows, sz_counts, sz_scal;     // sz_scal: [0] non-zero bins of a flush (distinct rows of a log), [1] rows appended by it
    DevBuf lr_table;                        // wk_log_reduce: [slots] row indices, then [slots] counts
    int64_t sz_n = 0, sz_flushes = 0;       // rows held; flushes that added some
    // read size per record of the staged chunk + reads the histogram does not
    // cover + totals: [0] derived at staging, [1] derived again with the
    // validity bits of the current subject rows (when some subject has one set)
    DevBuf c_rk[2], rk_left[2], rk_totals;
    bool rk_valid[2] = {false, false};
    int64_t rk_reads[2] = {0, 0}, rk_records[2] = {0, 0};
    int64_t stage_serial = 0, rows_serial = 0, rk1_stage = -1, rk1_rows = -1;
    int64_t stat_extra_reads = 0, stat_extra_records = 0;  // statistics added on the host
    bool rows_any_invalid = false;  // some subject lacks an ancestor at a rank column of the current rows
    // packed records of the native tokenizer accumulated over the chunks of one
    // sample (wk_words_*): one launch of the weighted histogram at the end
    DevBuf c_words;   // (per-read stream, w_mode != 0: one buffer, reads contiguous)
    // weighted histogram (w_mode 0): the records by slice of the subject table (wk_weigh.hpp), appended through device
    // cursors; unsliced (more than kMaxStreams slices) = one stream for the team kernel
    DevBuf w_stream[kMaxStreams], w_cursor, w_stage, w_backup, w_backup2;
    void* w_backup_cur = nullptr;   // the cursors in front of the block emitted last (what a block that is not kept restores)
    bool fz_chain = false;          // the one-kernel tokenizer's last launch left the next block's "before" and cleared scalars behind
    int fz_parity = 0;              // ... in w_backup (0) / w_backup2 (1) / w_backup3 (2): `fz_bk(i)`
    DevBuf w_backup3;
    // blocks of the one-kernel tokenizer whose verdict has not been read yet (wk_dtok_scan_emit_begin / _end): at most
    // two, oldest first -- the second one's kernel is queued behind the first one's, so that the device never waits
    // for the host between blocks
    struct LagSlot {
        int buf = -1;                // text buffer (-1: a resident block)
        const char* src = nullptr;   // the block's tag (put back when the block is handed back)
        uint32_t n = 0;
        bool open_end = false;
        int ring = 0;                // fz_bk(ring) = the cursors in front of the block
        uint32_t lines_est = 0;
        int host_slot = 0;           // slot of the pinned scratch its scalars land in
        hipEvent_t ev = nullptr;
        uint32_t seq = 0;
    };
    LagSlot lag[2];
    int lag_count = 0;
    hipEvent_t lag_ev[2] = {nullptr, nullptr};
    int lag_next_ev = 0;
    int fz_back_streak = 0, fz_skip = 0;   // blocks in a row the one kernel handed back; blocks it is left out for
    bool count_ahead = true;        // wk_set_option "dtok_count_ahead"
    bool lag_poll = true;           // a block's end is seen in pinned memory instead of waited for through an event (WOLTKA_LAG_POLL=0: the event; 127.7 against 126.3 us per block, tools/lag_probe.py)
    uint32_t lag_seq = 0;
    bool lag_enabled = true;        // (WOLTKA_NO_LAG=1: every block's verdict is read before the next is launched)
    int w_streams = 0;              // streams the open accumulation writes to
    bool w_sliced = false;
    bool w_counts_known = false;    // w_count holds the cursors' values
    unsigned long long w_count[kMaxStreams] = {};
    int64_t w_records = 0, w_reads = 0;  // accumulated so far
    std::vector<wk_job> w_jobs;          // the job set they will be classified under
    int32_t w_group = 0;
    bool w_open = false;
    // host memory of others registered for asynchronous copies (wk_host_register): a copy may not span two of them
    struct HostReg {
        const char* p;
        size_t n;
    };
    std::mutex reg_mu;
    std::vector<HostReg> regs;
    int w_mode = 0;  // 0: subject indices for the weighted histogram; the stream of wk_free.hpp: 1: feature ids (one free-rank job), 2: ancestors at the job's rank (one rank job under --uniq / --above / --major), 3: subject indices, rewritten per job when the sample is classified (several such jobs), 4: subject indices read by both evaluators (whole-read jobs next to plain ones: wk_words_begin_mixed)
    bool w_mixed_entry = false;  // the accumulation was opened by wk_words_begin_mixed (words_roll re-opens it there)
    int rank_serial = 0;              // bumped by wk_build_rank_table
    int free_per_cu = 2, free_threads = 1024, free_slots = 4096;  // launch shape of the free-rank stream (measurement knobs; DESIGN_HISTORY §3.1d)  // measurement knobs of the free-rank stream: workgroups per CU, windows in flight per wave
    int32_t max_gene_feature = 0;
    int use_range_log = 1;  // (0: the hashed miss log for the gene tally too; measurement)
    int words_keep = 0;  // measurement: wk_words_flush leaves the accumulated records in place
    static constexpr int kStageSlots = 8;
    hipEvent_t slot_ev[kStageSlots] = {};
    bool slot_busy[kStageSlots] = {};
    std::vector<void*> host_blocks;      // wk_host_alloc (guarded by host_mu: the host layer pins buffers on several threads)
    std::mutex host_mu;
    // device tokenizer (wk_dtok.hpp): the block scanned last and the dictionary mirror
    // the block being scanned + the blocks copied ahead of it.  Three are enough while the scans keep up with
    // the link; the host layer's reader may start before anything can be scanned (the hierarchy is still
    // being read) and then runs as far ahead as it likes -- HBM is what a 288 GB device has to spare; the
    // buffers are allocated as they are first used, the lowest free one first
    static constexpr int kTextBufs = 192;
    // (text buffers are cut from slabs of kSlabBufs: one hipMalloc per GB instead of one per block while the reader
    // runs ahead -- every allocation holds the runtime's lock against the launches of the scans; a block larger than a
    // slab's share gets a buffer of its own, TextBuf::own)
    static constexpr int kSlabBufs = 16;
    static constexpr size_t kTextStride = ((size_t)66 << 20) + 256;
    DevBuf d_textslab[kTextBufs / kSlabBufs];
    enum : unsigned char { kBufFree = 0, kBufCopied = 1, kBufScanning = 2, kBufPending = 3 };
    TextBuf text_buf[kTextBufs];
    std::mutex copy_mu;   // the text buffers' states and tags (see TextBuf)
    std::mutex slab_mu;   // a slab is allocated by whoever needs one of its buffers first
    unsigned long long copy_seq_next = 1;
    // what kernels write about the blocks copied ahead, in pinned memory, by text buffer: the newlines of a block
    // counted behind its copy, the inflate kernel's "a member failed" word
    unsigned long long* copy_newlines = nullptr;   // [kTextBufs], behind the slots of host_back
    uint32_t* di_any_host = nullptr;               // [kTextBufs], allocated by the first wk_dtok_inflate_ahead
    DevBuf d_tiles, d_tile_off, d_lines, d_lsubj, d_lmeta, d_start, d_first, d_unknown, d_state, d_dict, d_dict2, d_names16, d_arena, d_submap;
    DevBuf d_timeline;         // (measurement, wk_dtok_fused_timeline) the stamps of the measuring instance's sampled workgroups
    uint32_t tl_wgs = 0;       // ... of the launch that wrote them last: its sampled workgroups
    bool dt_mapped = false;       // the block scanned last has had its lines' ids translated (dtok_submap_kernel)
    bool dt_submap_on = false;    // a map has been given (it may be empty still)
    bool dt_has_excl = false;     // the map holds kLineExcluded: `--exclude` on the device text route
    uint32_t dt_submap_n = 0;     // wk_dtok_subject_map (0: the tokenizer's ids are the subject indices)
    DevBuf d_lbeg, d_lend, d_llen, d_lscan, d_gmap;  // "ex" flavour
    bool dt_extra = false;
    // coverage pile (wk_cover.hpp): two buffers of rows (the sort's ping-pong; cv_cur holds the pile), the merged set
    // of the sample so far in front of the rows appended since
    DevBuf cv_key[2], cv_end[2], cv_reach, cv_hist, cv_tiles, cv_tile_off, cv_state, cv_stage[3];
    bool cv_open = false;
    int cv_cur = 0;
    int64_t cv_cap = 0;       // rows a buffer holds
    int64_t cv_cap_opt = 0;   // wk_set_option("cover_cap_rows"): what wk_cover_begin(ctx, 0) reserves (0: kCoverCapDefault)
    int64_t cv_tail = 0;      // rows in the pile, the merged set included
    int64_t cv_merged = 0;    // rows of the merged set
    int64_t cv_ub = 0;        // upper bound of the tail: cv_tail + the lines handed to cover_append since it was read
    bool cv_stale = false;    // rows have been appended since cv_tail / cv_seen were read
    CoverState cv_seen{};     // the device's scalars as read last
    uint32_t cv_line_next = 0;  // lines of the block scanned last that wk_dtok_cover_append has been through
    // measurement (woltka_hip_measure.h): blocks of text that are resident on the device already
    // (wk_text_upload) -- the scan of such a block copies nothing
    struct ResidentText {
        const char* host;
        uint32_t n;
        unsigned char* dev;
        unsigned long long* tile_off;  // the block's newline offsets per tile, counted at upload
        unsigned long long n_newlines;
    };
    std::vector<ResidentText> resident;
    // gzip members inflated on the device (wk_dinflate.hpp): the compressed bytes, the members' spans, the text and
    // the status words of wk_inflate_members_device
    DevBuf di_blob, di_meta, di_out, di_status;   // (those of the blocks wk_dtok_inflate_ahead fills: TextBuf)
    const unsigned char* dt_text = nullptr;  // the text of the block scanned last
    int dt_fmt = 0;   // WK_FMT_* of the blocks (wk_dtok_format)
    uint32_t dt_n = 0, dt_lines = 0, dt_dict_mask = 0;
    int32_t dt_dict_names = -1;  // names of the tokenizer the mirror holds
    const wk_tok* dt_dict_tok = nullptr;
    bool dt_ready = false;
    // the text of a block is copied on a stream of its own into a free text buffer while the kernels work on the
    // buffers of the blocks before it (wk_dtok_copy); its newlines are counted behind the copy on another
    hipStream_t copy_stream = nullptr, count_stream = nullptr;
    bool dt_detached = false;         // the block scanned last: its host bytes are gone (TextBuf::detached)
    // (wk_dtok_expect) bytes of text the open sample will have brought in all; the records that makes, told from
    // the first block's lines per byte: the sample's record buffers are sized once instead of doubled eight times
    int64_t dt_expect_bytes = 0, w_expect = 0;
    // Small results of a block (its DtokState, totals) come back through pinned memory that a one-wave kernel
    // writes (small_back): a hipMemcpyAsync of a few bytes queues on the DMA engine behind the 64 MB text copy
    // that is under way there, and the scan loop then runs at the pace of the link instead of the kernels'
    unsigned char* host_back = nullptr;   // [kBackSlots][kBackBytes] pinned, then copy_newlines[kTextBufs]
    static constexpr int kBackSlots = 4, kBackBytes = 256;
    // read maps formatted on the device (wk_readmap.hpp): per job the taxon slot of every subject, the slots' order
    // and shown text; per block the reads' leader lines, line lengths / offsets and the text itself
    struct MapTables {
        DevBuf slot_of_subject, slot_order, shown_off, shown;
        int32_t n_subjects = 0, n_slots = 0;
    };
    MapTables rm[WK_MAX_JOBS];
    DevBuf rm_line, rm_len, rm_text;
    // strata map of the current sample on the device (wk_strata.hpp)
    DevBuf s_text, s_lines, s_tab, s_vlen, s_hash, s_label, s_slots, s_labels, s_label_text, s_label_group, s_state, s_tiles, s_tile_off;
    uint32_t s_n = 0, s_n_lines = 0, s_mask = 0;
    bool s_ready = false;   // wk_strata_load built the tables
    bool s_use = false;     // wk_strata_groups gave the labels their groups: wk_dtok_stage_hits joins
    // demultiplexing on the device (wk_demux.hpp): the sample table (its host mirror is what is uploaded), the block's pending names
    DevBuf dx_tab, dx_name_off, dx_arena, dx_group, dx_met, dx_pend, dx_pend_list, dx_state, dx_lsamp, dx_out;
    std::vector<DemuxSlot> dx_tab_host;
    std::vector<uint2> dx_name_off_host;
    std::vector<unsigned char> dx_arena_host;
    std::vector<int64_t> dx_pend_off;     // the pending names of the block scanned last, in order of their first read ...
    std::vector<int32_t> dx_pend_len;
    std::vector<char> dx_pend_blob;       // ... and their bytes
    bool dx_on = false;                   // wk_demux_begin
    bool dx_looked = false;               // wk_demux_pending has looked the scanned block's samples up
    bool dx_runs = false;                 // ... and its run starts are told, its subject map and exclusion set applied
    int dx_status = 1;                    // ... and what it found
    bool dx_chunk = false;                // the staged chunk is wk_dtok_stage_reads' or wk_dtok_stage_reads_strata's
    bool dx_hits = false;                 // the staged hits are wk_dtok_stage_hits_demux': the match marks the samples met
    DevBuf dx_rsamp;                      // ... and the sample id of every read of theirs (-1: not in the table)
    int32_t dx_groups_n = 0;              // samples that have a group (wk_demux_register)
    uint64_t dx_hash_mask = 0;            // (tests) option "demux_hash_mask"
    int64_t dx_max_opt = 0;               // (tests) option "demux_max_samples"
    bool dt_keep_reads = false;   // wk_dtok_keep_reads: wk_dtok_emit places the records in read order and keeps the block
    bool dt_emitted = false;      // the block scanned last was emitted with its reads kept
    uint32_t dt_emit_reads = 0;
    int64_t rm_bytes = 0;         // text of the last wk_dtok_readmap / wk_dtok_readmap_reads
    // read maps of whole-read assignments (wk_readmap_reads.hpp): the shown-text table over the feature ids, the
    // kernels' flags; what the codes wk_classify_staged_keep left in assign_out belong to
    DevBuf rr_off, rr_text, rr_flags;
    int32_t rr_n = 0;             // features the table covers
    uint32_t rr_text_n = 0;       // bytes of their text
    bool rr_chunk = false;        // the staged chunk is wk_dtok_stage_reads_plain's: its reads' leader lines are in rm_line
    int64_t rr_serial = -1;       // stage_serial of the chunk whose codes assign_out holds ...
    int32_t rr_jobs = 0;          // ... and the jobs they were written for
    uint32_t rr_unassigned = 0;   // ... under --unassigned
    // read maps with taxon lists (wk_readmap_lists.hpp): the id table the lists are ordered by when the shown text is
    // not the id, the lists' pairs; the kind of every job the codes were written for
    DevBuf rl_off, rl_text, rl_pairs, rl_npairs;
    int32_t rl_n = 0;             // features the id table covers (0: the shown text is the id)
    uint32_t rl_text_n = 0;
    int32_t rl_mode[WK_MAX_JOBS] = {};
    int32_t rl_slot[WK_MAX_JOBS] = {};
    // read maps under demultiplexing (wk_readmap_demux.hpp): the sample id of every read of the staged chunk, the
    // samples' columns, the partition's matrix, column bases, segment table and the lines' places
    DevBuf rd_samp, pd_present, pd_state, pd_mat, pd_col, pd_seg, pd_off;
    bool rd_chunk = false;        // the staged chunk is wk_dtok_stage_reads_samples': rd_samp, rm_line and the columns are its reads'
    uint32_t rd_cols = 0;         // ... and the samples it holds
    int32_t rd_segs = 0;          // segments of the text wk_dtok_readmap_*_demux made last
    int64_t pd_cap_opt = 0;       // option "readmap_demux_cap": entries of the matrix (0: kPartCapDefault)
    int range_parts_opt = 0;   // partitions of the dense gene log (0: as few as the merge's LDS array allows; measurement)
    int use_streams = 1;   // (0: the records of all slices in one stream, round 3's team kernel; measurement)
    int use_subject_bins = 1;
    int use_hot_bins = 1;  // hot-subject bins for subject tables beyond the LDS  // count-first mode of the split for small subject tables
};

namespace {

int fail(wk_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_last_error = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail((ctx), WK_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                        __FILE__, __LINE__);                                                     \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
};

constexpr int kStatBlocks = 16384;  // >= the largest classify grid (256 CUs x 32 + slack)

unsigned long long* scalar_u64(wk_ctx* c, int idx) { return c->scalars.as<unsigned long long>() + idx; }
int* scalar_err(wk_ctx* c) { return c->scalars.as<int>(); }

// Device memory for text buffer k, at least `need` bytes.
hipError_t text_buffer(wk_ctx* c, int k, size_t need) {
    if (need <= wk_ctx::kTextStride) {
        DevBuf& slab = c->d_textslab[k / wk_ctx::kSlabBufs];
        std::lock_guard<std::mutex> lock(c->slab_mu);
        if (!slab.p) {
            const hipError_t e = slab.reserve(wk_ctx::kTextStride * wk_ctx::kSlabBufs);
            if (e != hipSuccess) return e;
        }
        c->text_buf[k].text = slab.as<unsigned char>() + (size_t)(k % wk_ctx::kSlabBufs) * wk_ctx::kTextStride;
        return hipSuccess;
    }
    TextBuf& b = c->text_buf[k];
    const hipError_t e = b.own.reserve(need);
    if (e == hipSuccess) b.text = b.own.as<unsigned char>();
    return e;
}

// ---- the searches among the text buffers: each is called with copy_mu held --------------------------------------
// The oldest block copied ahead with this tag (a reader that reuses its pinned buffers may have copied two blocks of
// one length from one address); -1: none.
int textbuf_find_copied(const wk_ctx* c, const char* src, uint32_t n) {
    int k = -1;
    for (int q = 0; q < wk_ctx::kTextBufs; ++q) {
        const TextBuf& b = c->text_buf[q];
        if (b.state == wk_ctx::kBufCopied && b.src == src && b.n == n && (k < 0 || b.seq < c->text_buf[k].seq)) k = q;
    }
    return k;
}

// Buffer k goes over to `state` and is found by no tag any more.
void textbuf_claim(wk_ctx* c, int k, unsigned char state) {
    TextBuf& b = c->text_buf[k];
    b.state = state;
    b.src = nullptr;
    b.counted = false;
}

// The lowest free buffer, claimed for `state`; -1: none is free.
int textbuf_take_free(wk_ctx* c, unsigned char state) {
    for (int q = 0; q < wk_ctx::kTextBufs; ++q)
        if (c->text_buf[q].state == wk_ctx::kBufFree) {
            textbuf_claim(c, q, state);
            c->text_buf[q].detached = false;
            return q;
        }
    return -1;
}

// The buffer of the block scanned last is free once the next scan begins: its kernels have been waited for.
void textbuf_release_scanned(wk_ctx* c) {
    for (TextBuf& b : c->text_buf)
        if (b.state == wk_ctx::kBufScanning) b.state = wk_ctx::kBufFree;
}

// Buffer k holds a block copied ahead again (its text is where it was, its newlines count as not counted).
void textbuf_retag(wk_ctx* c, int k, const char* src, uint32_t n) {
    TextBuf& b = c->text_buf[k];
    b.state = wk_ctx::kBufCopied;
    b.src = src;
    b.n = n;
    b.counted = false;
}

// `bytes` (<= 256, a multiple of 4) from device memory to pinned host memory, by the device itself
__global__ void small_back_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ host, uint32_t words) {
    if (threadIdx.x < words) host[threadIdx.x] = src[threadIdx.x];
}

// (one word to device memory without a trip through the DMA queue)
__global__ void store_u32_kernel(uint32_t* dst, uint32_t value) { *dst = value; }

// Queue the copy of a small result into slot `slot` of the pinned scratch; read it with small_back_get once the
// stream has been waited for.
hipError_t small_back(wk_ctx* c, int slot, const void* dev, size_t bytes) {
    if (!c->host_back || slot < 0 || slot >= wk_ctx::kBackSlots || bytes > (size_t)wk_ctx::kBackBytes || (bytes & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(small_back_kernel, dim3(1), dim3(64), 0, c->stream, static_cast<const uint32_t*>(dev),
                       reinterpret_cast<uint32_t*>(c->host_back + (size_t)slot * wk_ctx::kBackBytes), (uint32_t)(bytes / 4));
    return hipGetLastError();
}
void small_back_get(wk_ctx* c, int slot, void* out, size_t bytes) {
    std::memcpy(out, c->host_back + (size_t)slot * wk_ctx::kBackBytes, bytes);
}

struct Lap {
    double* acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit Lap(double* a) : acc(a) {}
    ~Lap() { *acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

// start of an API call that times its kernels: a fresh head of the chain
void ktimer_step(wk_ctx* c) {
    if (!c->profile) return;
    if (!c->kt_step && hipEventCreate(&c->kt_step) != hipSuccess) {
        c->kt_step = nullptr;
        return;
    }
    (void)hipEventRecord(c->kt_step, c->stream);
    c->kt_tail = c->kt_step;
}
// (API calls nest — wk_ordinal_count runs wk_classify_staged —: the outermost one heads the chain)
struct KtScope {
    wk_ctx* c;
    explicit KtScope(wk_ctx* ctx) : c(ctx) {
        if (c->kt_depth++ == 0) ktimer_step(c);
    }
    ~KtScope() { --c->kt_depth; }
};
KernelTimer* ktimer_begin(wk_ctx* c, const char* family) {
    if (!c->profile) return nullptr;
    if (!c->kt_tail) ktimer_step(c);
    if (!c->kt_tail) return nullptr;
    KernelTimer& t = c->ktimers[family];
    if (!t.b && hipEventCreate(&t.b) != hipSuccess) {
        t.b = nullptr;
        return nullptr;
    }
    t.valid = false;
    // (a family launched twice in a call: its second bracket would start at its own event, which is about to be recorded again)
    t.from = c->kt_tail == t.b ? c->kt_step : c->kt_tail;
    return &t;
}
void ktimer_end(wk_ctx* c, KernelTimer* t) {
    if (!t) return;
    (void)hipEventRecord(t->b, c->stream);
    c->kt_tail = t->b;
    t->valid = true;
}

int check_device_errors(wk_ctx* c) {
    int e = 0;
    HIP_TRY(c, hipMemcpyAsync(&e, scalar_err(c), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (e == 0) return WK_OK;
    HIP_TRY(c, hipMemsetAsync(scalar_err(c), 0, sizeof(int), c->stream));
    if (e & kErrTableFull) return fail(c, WK_E_TABLE_FULL, "count table is full (%llu slots); call wk_counts_reserve with more slots", (unsigned long long)c->slots);
    if (e & kErrKRange) return fail(c, WK_E_RANGE, "a read has more than %d candidate features", WK_MAX_K);
    if (e & kErrFeatureRange) return fail(c, WK_E_RANGE, "feature id outside [0, %d]", WK_MAX_FEATURE);
    if (e & kErrGroupRange) return fail(c, WK_E_RANGE, "group id outside [0, %d)", 1 << WK_KEY_GROUP_BITS);
    if (e & kErrPairOverflow) return fail(c, WK_E_RANGE, "more than 2^31 read-gene pairs in one chunk");
    return fail(c, WK_E_HIP, "unknown device error flag %d", e);
}

int upload(wk_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    HIP_TRY(c, b.reserve(bytes ? bytes : 1));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return WK_OK;
}

// reads per thread and round in the per-read first pass (classify_single_kernel)
constexpr int kPerReadItems = 2;

int grid_for(int64_t n, int threads, int max_blocks) {
    int64_t b = (n + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

__global__ void __launch_bounds__(256) table_count_kernel(const unsigned long long* __restrict__ keys,
                                                          uint64_t slots, unsigned long long* __restrict__ n) {
    unsigned long long mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
        mine += (keys[i] != kEmptyKey) ? 1ull : 0ull;
    mine = wave_sum(mine);
    if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(n, mine);
}

__global__ void __launch_bounds__(256) table_compact_kernel(const unsigned long long* __restrict__ keys,
                                                            const unsigned long long* __restrict__ vals,
                                                            uint64_t slots, unsigned long long* __restrict__ cursor,
                                                            unsigned long long* __restrict__ out_k,
                                                            long long* __restrict__ out_v) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (slots + stride - 1) / stride;
    const int lane = threadIdx.x & (kWave - 1);
    for (uint64_t it = 0; it < rounds; ++it) {  // wave-uniform trip count: ballots see all lanes
        const uint64_t i = it * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const unsigned long long k = (i < slots) ? keys[i] : kEmptyKey;
        const bool live = (k != kEmptyKey);
        const unsigned long long m = __ballot(live);
        if (m == 0) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, kWave);
        if (live) {
            const unsigned long long pos = base + __popcll(m & ((1ull << lane) - 1ull));
            out_k[pos] = k;
            out_v[pos] = (long long)vals[i];
        }
    }
}

}  // namespace

// tree.find_rank (tree.py:467-510) for the subjects, on the host: ancestor (or
// self) of each subject's node with the rank code of `slot`, -1 if none — what
// rank_table_kernel holds for all nodes.  Kept up to date as subjects are added.
static int ensure_subject_ancestors(wk_ctx* c, wk_ctx::StreamTables& T, int slot) {
    std::vector<int32_t>& t = T.subj_node_host;
    if (T.node_slot != slot || T.node_tree != c->tree_serial || T.node_rank != c->rank_serial) t.clear();
    if ((int32_t)t.size() > c->n_subjects) t.clear();
    const size_t have = t.size();
    if (have == (size_t)c->n_subjects && T.node_slot == slot) return WK_OK;
    const int32_t code = c->rank_tab_code[slot];
    t.resize((size_t)c->n_subjects, -1);
    for (size_t s = have; s < t.size(); ++s) {
        int32_t u = c->subj_feat_host[s], res = -1;
        if (u < c->n_nodes)
            for (;;) {
                if (c->rank_code_host[u] == code) {
                    res = u;
                    break;
                }
                const int32_t p = c->parent_host[u];
                if (p == u) break;
                u = p;
            }
        t[s] = res;
    }
    T.node_slot = slot;
    T.node_tree = c->tree_serial;
    T.node_rank = c->rank_serial;
    const int rc = upload(c, T.subj_node, t.data(), t.size() * 4);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// The nodes the records of the per-read stream (wk_free.hpp) can name — the
// subjects' nodes (mode 1, `--rank free`) or their ancestors at the job's rank
// (mode 2) — and every subject's place among them.  `before` (optional) receives
// the list as it was when a list for the same job over the same tree is replaced
// (the subject table has grown): records written under it are renumbered.
static int ensure_rank_table(wk_ctx* c, wk_ctx::StreamTables& T, int mode, int slot, std::vector<int32_t>* before) {
    if (mode == 2) {
        const int rc = ensure_subject_ancestors(c, T, slot);
        if (rc) return rc;
    }
    if (T.rk_kind == mode && T.rk_slot == slot && T.rk_tree == c->tree_serial && T.rk_subj == c->subj_serial && T.rk_rank == c->rank_serial)
        return WK_OK;
    const int32_t n_nodes = c->n_nodes;
    const std::vector<int32_t>& of = mode == 2 ? T.subj_node_host : c->subj_feat_host;
    std::vector<int32_t> dn;  // distinct nodes, ascending
    dn.reserve(of.size());
    for (int32_t v : of)
        if (v >= 0 && v < n_nodes) dn.push_back(v);
    std::sort(dn.begin(), dn.end());
    dn.erase(std::unique(dn.begin(), dn.end()), dn.end());
    std::vector<int32_t> rank_of(of.size(), -1);
    for (size_t s = 0; s < of.size(); ++s)
        if (of[s] >= 0 && of[s] < n_nodes) rank_of[s] = (int32_t)(std::lower_bound(dn.begin(), dn.end(), of[s]) - dn.begin());
    const int rc = upload(c, T.subj_rank, rank_of.data(), rank_of.size() * 4);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the vector is about to go out of scope)
    const bool same_job = T.rk_kind == mode && T.rk_slot == slot && T.rk_tree == c->tree_serial && T.rk_rank == c->rank_serial;
    if (before) {
        before->clear();
        if (same_job) before->swap(T.dn_host);
    }
    T.dn_host.swap(dn);
    T.rk_kind = mode;
    T.rk_slot = slot;
    T.rk_tree = c->tree_serial;
    T.rk_subj = c->subj_serial;
    T.rk_rank = c->rank_serial;
    return WK_OK;
}

// Tables of the per-read stream over those nodes: the parents, the table of neighbours' LCAs.
static int ensure_stream_tables(wk_ctx* c, wk_ctx::StreamTables& T, int mode, int slot) {
    {
        const int rc = ensure_rank_table(c, T, mode, slot, nullptr);
        if (rc) return rc;
    }
    if (T.kind == mode && T.slot == slot && T.tree == c->tree_serial && T.subj == c->subj_serial && T.rank == c->rank_serial)
        return WK_OK;
    const int32_t n_nodes = c->n_nodes;
    const std::vector<int32_t>& dn = T.dn_host;
    const uint32_t md = (uint32_t)dn.size();
    uint32_t dlevels = 1;
    while (md > 1 && (2u << (dlevels - 1)) <= md - 1) dlevels += 1;
    const size_t drow = std::max<uint32_t>(md, 1u);
    // ... in terms of *result ids*: the nodes a read can be assigned to are the
    // subject nodes and their ancestors (a few hundred thousand of a 2 M-node
    // tree), numbered in pre-order — so that the smallest id is still the
    // shallowest ancestor, and the root is 0 — to keep the stream's counters
    // (one per possible result) small enough to stay in the L2s
    std::vector<int32_t> rid((size_t)std::max(n_nodes, 1), -1);
    for (int32_t v : dn)
        for (int32_t u = v; rid[(size_t)u] < 0; u = c->parent_host[u]) {
            rid[(size_t)u] = 0;
            if (c->parent_host[u] == u) break;
        }
    std::vector<int32_t> rnode;
    for (int32_t v = 0; v < n_nodes; ++v)
        if (rid[(size_t)v] == 0) {
            rid[(size_t)v] = (int32_t)rnode.size();
            rnode.push_back(v);
        }
    if (rnode.empty()) rnode.push_back(0);
    std::vector<int32_t> dsparse(drow * dlevels, 0x7FFFFFFF), dparent(drow, -1), dself(drow, -1);
    for (uint32_t i = 0; i < md; ++i) {
        dparent[i] = rid[(size_t)c->parent_host[dn[i]]];
        dself[i] = rid[(size_t)dn[i]];
    }
    for (uint32_t i = 0; i + 1 < md; ++i) {
        int32_t u = dn[i];
        while (c->last_host[u] < dn[i + 1]) u = c->parent_host[u];
        dsparse[i] = rid[(size_t)u];
    }
    for (uint32_t k = 1; k < dlevels; ++k)
        for (uint32_t i = 0; i + (1u << k) <= md - 1; ++i)
            dsparse[k * drow + i] = std::min(dsparse[(k - 1) * drow + i], dsparse[(k - 1) * drow + i + (1u << (k - 1))]);
    int rc;
    if ((rc = upload(c, T.dsparse, dsparse.data(), dsparse.size() * 4))) return rc;
    if ((rc = upload(c, T.dparent, dparent.data(), dparent.size() * 4))) return rc;
    if ((rc = upload(c, T.dself, dself.data(), dself.size() * 4))) return rc;
    if ((rc = upload(c, T.rnode, rnode.data(), rnode.size() * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the vectors are about to go out of scope
    T.results = (uint32_t)rnode.size();
    T.dm = (uint32_t)drow;
    T.kind = mode;
    T.slot = slot;
    T.tree = c->tree_serial;
    T.subj = c->subj_serial;
    T.rank = c->rank_serial;
    return WK_OK;
}

// Tables behind ClassifyArgs::free_sparse for the current tree and subject
// table (host side: 100 k subjects x ~17 levels).
static int ensure_free_tables(wk_ctx* c) {
    if (c->free_tree == c->tree_serial && c->free_subj == c->subj_serial) return WK_OK;
    const int32_t n = c->n_subjects, n_nodes = c->n_nodes;
    const std::vector<int32_t>& feat = c->subj_feat_host;
    std::vector<int32_t> order;
    order.reserve((size_t)n);
    for (int32_t s = 0; s < n; ++s)
        if (feat[s] < n_nodes) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return feat[x] < feat[y] || (feat[x] == feat[y] && x < y); });
    const uint32_t m = (uint32_t)order.size();
    std::vector<int32_t> rank((size_t)std::max(n, 1), -1);
    for (uint32_t i = 0; i < m; ++i) rank[order[i]] = (int32_t)i;
    uint32_t levels = 1;
    while (m > 1 && (2u << (levels - 1)) <= m - 1) levels += 1;  // the longest range of pairs has m - 1 of them
    const size_t row = std::max<uint32_t>(m, 1u);
    std::vector<int32_t> sparse(row * levels, 0x7FFFFFFF);
    for (uint32_t i = 0; i + 1 < m; ++i) {  // LCA of neighbours: the lowest ancestor of the first whose subtree holds the second
        int32_t u = feat[order[i]];
        const int32_t hi = feat[order[i + 1]];
        while (c->last_host[u] < hi) u = c->parent_host[u];
        sparse[i] = u;
    }
    for (uint32_t k = 1; k < levels; ++k)
        for (uint32_t i = 0; i + (1u << k) <= m - 1; ++i)
            sparse[k * row + i] = std::min(sparse[(k - 1) * row + i], sparse[(k - 1) * row + i + (1u << (k - 1))]);
    int rc;
    if ((rc = upload(c, c->f_rank, rank.data(), rank.size() * 4))) return rc;
    if ((rc = upload(c, c->f_sparse, sparse.data(), sparse.size() * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the vectors are about to go out of scope
    c->f_m = (uint32_t)row;
    c->free_tree = c->tree_serial;
    c->free_subj = c->subj_serial;
    return WK_OK;
}

// Read size per record of the staged chunk (wk_weigh.hpp): marks at the read
// starts, then spread over the records.  `check`: leave out reads that name a
// subject with its validity bit set.
static int derive_read_sizes(wk_ctx* c, bool check, const int32_t* qoff, const int32_t* subj, int64_t n_reads, int64_t n_rec,
                             unsigned char* rk, unsigned long long* left, unsigned long long* totals) {
    HIP_TRY(c, hipMemsetAsync(totals, 0, 16, c->stream));
    HIP_TRY(c, hipMemsetAsync(rk + n_rec, 0, 8, c->stream));  // the sizes are read four at a time
    const int64_t n_tiles = (n_reads + kSizeTile - 1) / kSizeTile;
    const dim3 grid((unsigned)std::min<int64_t>(n_tiles, (int64_t)c->prop.multiProcessorCount * 2));
    if (check)
        hipLaunchKernelGGL(read_sizes_kernel<true>, grid, dim3(kSizeTile), 0, c->stream, qoff, (uint32_t)n_reads, subj,
                           c->w_invalid.as<uint32_t>(), (uint32_t)c->n_subjects, rk, left, totals);
    else
        hipLaunchKernelGGL(read_sizes_kernel<false>, grid, dim3(kSizeTile), 0, c->stream, qoff, (uint32_t)n_reads, subj,
                           (const uint32_t*)nullptr, 0u, rk, left, totals);
    HIP_TRY(c, hipGetLastError());
    return WK_OK;
}

// Subject rows {feature, ancestor at rank column 0, 1, ...} for a job set over
// the current subject table (rebuilt when the subjects or the rank tables
// changed), the jobs' columns, and which subjects the weighted histogram cannot
// take (c->rows_any_invalid).
static int build_subject_rows(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, ClassifyArgs& a) {
    // (re)build the compact subject rows for this set of rank tables
    if (c->n_subjects <= 0 && c->n_records > 0) return fail(c, WK_E_STATE, "chunk carries subject indices but no subject table is set (wk_set_subjects)");
    std::vector<int> sig;
    RowCols cols{};
    for (int j = 0; j < n_jobs; ++j) {
        if (jobs[j].mode != WK_MODE_RANK) continue;
        int col = -1;
        for (int q = 0; q < cols.n_cols; ++q)
            if (sig[q] == jobs[j].rank_slot) col = q;
        if (col < 0) {
            col = cols.n_cols++;
            sig.push_back(jobs[j].rank_slot);
            cols.anc[col] = c->rank_tab[jobs[j].rank_slot].as<int32_t>();
        }
        a.jobs[j].col = col;
    }
    // `--rank free`: one more column with the subject's rank among the
    // subjects of the tree, when it fits the 4-column row
    bool any_free = false;
    for (int j = 0; j < n_jobs; ++j) any_free |= jobs[j].mode == WK_MODE_FREE;
    cols.by_subject = -1;
    int free_col = -1;
    // (the table has n log n entries: subject tables beyond 4 M keep the walk)
    if (any_free && c->use_free_sparse && cols.n_cols < 3 && c->n_subjects > 0 && c->n_subjects <= (1 << 22) && c->n_nodes > 0) {
        int rc2 = ensure_free_tables(c);
        if (rc2) return rc2;
        free_col = cols.n_cols++;
        sig.push_back(-2);
        sig.push_back(c->free_tree);
        sig.push_back(c->free_subj);
        cols.anc[free_col] = nullptr;
        cols.by_subject = free_col;
        cols.subject_col = c->f_rank.as<int32_t>();
        a.free_sparse = c->f_sparse.as<int32_t>();
        a.free_m = (int32_t)c->f_m;
        a.free_col = free_col;
    }
    int w = 4;  // {feature, <= 3 rank columns}: the kernel's single-pass fast path
    while (w < 1 + cols.n_cols) w <<= 1;
    sig.push_back(-1);
    sig.push_back(c->n_subjects);
    if (sig != c->rows_sig || w != c->rows_w) {
        HIP_TRY(c, c->subj_rows.reserve((size_t)std::max(c->n_subjects, 1) * w * sizeof(int32_t)));
        if (c->n_subjects > 0) {
            hipLaunchKernelGGL(subject_rows_kernel, dim3((c->n_subjects + 255) / 256), dim3(256), 0, c->stream,
                               c->subj_feat.as<int32_t>(), c->n_subjects, c->n_nodes, cols, w,
                               c->subj_rows.as<int32_t>());
            HIP_TRY(c, hipGetLastError());
        }
        c->rows_sig = sig;
        c->rows_w = w;
        // which subjects the weighted histogram cannot take (wk_weigh.hpp)
        c->rows_any_invalid = false;
        c->rows_serial += 1;
        if (c->n_subjects > 0) {
            HIP_TRY(c, c->w_invalid.reserve(((size_t)c->n_subjects / 32 + 2) * 4));
            HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 6), 0, 8, c->stream));
            hipLaunchKernelGGL(subject_invalid_kernel, dim3((c->n_subjects + 255) / 256), dim3(256), 0, c->stream,
                               c->subj_rows.as<int32_t>(), w, cols.n_cols, c->n_subjects,
                               c->w_invalid.as<uint32_t>(), reinterpret_cast<uint32_t*>(scalar_u64(c, 6)));
            HIP_TRY(c, hipGetLastError());
            uint32_t any = 0;
            HIP_TRY(c, hipMemcpyAsync(&any, scalar_u64(c, 6), 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->rows_any_invalid = any != 0;
        }
    }
    a.rows = c->subj_rows.as<int32_t>();
    a.row_w = w;
    a.n_subjects = c->n_subjects;
    return WK_OK;
}

extern "C" {

static int refresh_word_ranks(wk_ctx* c, int64_t count);
static int streams_needed(const wk_ctx* c) { return std::max(1, (int)(((int64_t)c->n_subjects + kSliceBins - 1) / kSliceBins)); }

// the accumulation is empty again
static int words_reset(wk_ctx* c) {
    c->w_records = c->w_reads = 0;
    c->w_expect = 0;
    c->w_open = false;
    c->w_counts_known = false;
    c->fz_chain = false;
    if (c->w_cursor.p) HIP_TRY(c, hipMemsetAsync(c->w_cursor.p, 0, kMaxStreams * 8, c->stream));
    return WK_OK;
}

int wk_words_flush(wk_ctx* c);
int wk_words_begin(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t group, int* ok);

int wk_abi_version(void) { return WK_ABI_VERSION; }

#ifndef WK_BUILD_ID
#define WK_BUILD_ID "unknown"
#endif
// (the tag is also what the build recipe looks for in the file's bytes)
static const char kBuildTag[] = "WK_BUILD_ID=" WK_BUILD_ID;
const char* wk_build_id(void) { return kBuildTag + 12; }

int wk_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

const char* wk_last_error(const wk_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int wk_device_pci_bus_id(int device, char* buf, size_t cap) {
    if (!buf || cap < 16) return fail(nullptr, WK_E_ARG, "bad arguments");
    const hipError_t e = hipDeviceGetPCIBusId(buf, (int)cap, device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, WK_E_HIP, "hipDeviceGetPCIBusId(%d) failed: %s", device, hipGetErrorString(e));
    }
    return WK_OK;
}

int wk_create(int device, wk_ctx** out) {
    if (!out) return fail(nullptr, WK_E_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, WK_E_HIP, "no HIP device available (%s); libwoltka_hip has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= ndev) return fail(nullptr, WK_E_ARG, "device %d out of range [0,%d)", device, ndev);
    wk_ctx* c = new (std::nothrow) wk_ctx();
    if (!c) return fail(nullptr, WK_E_HIP, "out of host memory");
    c->device = device;
    DeviceGuard guard(device);
    if ((e = hipGetDeviceProperties(&c->prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        // (the text route's two streams with it: made by the first wk_dtok_copy they cost the reader 40 ms of a call's
        // first 100 -- it runs beside the hierarchy's and the pread pool's threads by then --, here 6)
        (e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->count_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&c->t0)) != hipSuccess || (e = hipEventCreate(&c->t1)) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&c->host_back),
                           (size_t)wk_ctx::kBackSlots * wk_ctx::kBackBytes + (size_t)wk_ctx::kTextBufs * 8,
                           hipHostMallocDefault)) != hipSuccess ||
        (e = c->scalars.reserve(128)) != hipSuccess ||
        (e = hipMemsetAsync(c->scalars.p, 0, 128, c->stream)) != hipSuccess ||
        (e = c->stat_block.reserve((size_t)kStatBlocks * 16)) != hipSuccess ||
        (e = hipMemsetAsync(c->stat_block.p, 0, (size_t)kStatBlocks * 16, c->stream)) != hipSuccess) {
        int rc = fail(nullptr, WK_E_HIP, "context setup failed: %s", hipGetErrorString(e));
        wk_destroy(c);
        return rc;
    }
    c->copy_newlines = reinterpret_cast<unsigned long long*>(c->host_back + (size_t)wk_ctx::kBackSlots * wk_ctx::kBackBytes);
    // the LDS front cache needs more than the default 64 KiB dynamic LDS limit
    // (160 KiB per CU minus the kernels' few bytes of static LDS)
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&stripe_match_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStripeMatchLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&free_stream_kernel<false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&free_stream_kernel<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&free_stream_kernel<false, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&free_stream_kernel<true, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&free_log_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLogBins * 4))) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_kernel<true, false, 0>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_kernel<true, false, 1>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_kernel<true, false, 2>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_kernel<true, true, 0>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_kernel<true, true, 1>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_kernel<true, true, 2>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<true, true, 4>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&count_subjects_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<false, true, kPerReadItems>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<false, false, kPerReadItems>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<true, true, 2, false, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<true, false, 2, false, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<false, true, kPerReadItems, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_single_kernel<false, false, kPerReadItems, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<4>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<4, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<6, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<8, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<3>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<6>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_bins_kernel<8>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_streams_kernel<4>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_streams_kernel<6>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_streams_kernel<8>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_wide_kernel<4>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sized_bins_kernel<4>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBinsMaxLds)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&weigh_merge_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&classify_tiled_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&match_hits_kernel<true, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&match_hits_kernel<true, false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&range_merge_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess ||
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&partition_merge_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024)) != hipSuccess) {
        int rc = fail(nullptr, WK_E_HIP, "hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(e));
        wk_destroy(c);
        return rc;
    }
    // (measurement: WOLTKA_NO_FUSED=1 keeps every block of the text route on the six kernels of wk_dtok.hpp, for
    // whole `woltka classify` calls that cannot reach wk_tune)
    if (const char* nf = getenv("WOLTKA_NO_FUSED")) c->use_fused = (nf[0] && nf[0] != '0') ? 0 : 1;
    if (const char* nl = getenv("WOLTKA_NO_LAG")) c->lag_enabled = !(nl[0] && nl[0] != '0');
    if (const char* lp = getenv("WOLTKA_LAG_POLL")) c->lag_poll = lp[0] && lp[0] != '0';
    if (const char* sm = getenv("WOLTKA_STRIPES_MIN"))
        if (sm[0]) c->stripes_min_hits = std::max<long long>(0, atoll(sm));
    *out = c;
    return WK_OK;
}

void wk_destroy(wk_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    DevBuf* bufs[] = {&c->nodes, &c->rank_code, &c->gene4, &c->g_grid, &c->g_first, &c->g_goff, &c->g_shift,
                      &c->tkeys, &c->tvals, &c->c_subj, &c->c_qoff, &c->c_group, &c->o_genome, &c->o_beg,
                      &c->o_end, &c->o_len, &c->o_hoff, &c->o_cnt, &c->o_ub, &c->o_first2, &c->o_poff, &c->o_pairs, &c->o_qoff,
                      &c->o_tile_sum, &c->o_tile_off, &c->scalars, &c->stat_block, &c->log, &c->subj_feat, &c->subj_rows, &c->dense_slab, &c->plog, &c->plog_cnt, &c->left_mask, &c->left_list, &c->first_slab, &c->w_slab, &c->w_hi, &c->w_invalid, &c->sz_rows, &c->sz_counts, &c->sz_scal, &c->lr_table, &c->c_rk[0], &c->c_rk[1], &c->rk_left[0], &c->rk_left[1], &c->rk_totals, &c->f_rank, &c->f_sparse, &c->f_dense, &c->w_renum, &c->f_log, &c->f_log_cnt, &c->f_partial, &c->f_part_used, &c->w_tmp, &c->assign_out, &c->fetch_k, &c->fetch_v};
    for (DevBuf* b : bufs) b->release();
    for (wk_ctx::StreamTables& T : c->st)
        for (DevBuf* b : {&T.dsparse, &T.dparent, &T.dself, &T.rnode, &T.subj_node, &T.subj_rank}) b->release();
    c->c_words.release();
    for (DevBuf* b : {&c->di_blob, &c->di_meta, &c->di_out, &c->di_status}) b->release();
    for (DevBuf& b : c->w_stream) b.release();
    c->w_wide.release();
    c->w_wide_plan.release();
    c->w_backup2.release();
    c->w_backup3.release();
    for (hipEvent_t& e : c->lag_ev)
        if (e) (void)hipEventDestroy(e);
    for (TextBuf& b : c->text_buf) {
        for (DevBuf* d : {&b.tiles, &b.tile_off, &b.di_comp, &b.di_meta, &b.di_status, &b.own}) d->release();
        for (hipEvent_t ev : {b.ev, b.ev0, b.evm})
            if (ev) (void)hipEventDestroy(ev);
    }
    for (DevBuf& slab : c->d_textslab) slab.release();
    for (DevBuf* b : {&c->d_tiles, &c->d_tile_off, &c->d_lines, &c->d_lsubj, &c->d_lmeta, &c->d_start, &c->d_first, &c->d_unknown, &c->d_lbeg, &c->d_lend, &c->d_llen, &c->d_lscan, &c->d_gmap,
                      &c->d_state, &c->d_timeline, &c->d_dict, &c->d_dict2, &c->d_names16, &c->d_arena, &c->d_submap, &c->cv_key[0], &c->cv_key[1], &c->cv_end[0], &c->cv_end[1],
                      &c->cv_reach, &c->cv_hist, &c->cv_tiles, &c->cv_tile_off, &c->cv_state, &c->cv_stage[0], &c->cv_stage[1], &c->cv_stage[2],
                      &c->dx_tab, &c->dx_name_off, &c->dx_arena, &c->dx_group, &c->dx_met, &c->dx_pend, &c->dx_pend_list, &c->dx_state, &c->dx_lsamp, &c->dx_out, &c->dx_rsamp,
                      &c->rr_off, &c->rr_text, &c->rr_flags,
                      &c->rl_off, &c->rl_text, &c->rl_pairs, &c->rl_npairs,
                      &c->rd_samp, &c->pd_present, &c->pd_state, &c->pd_mat, &c->pd_col, &c->pd_seg, &c->pd_off})
        b->release();
    for (wk_ctx::ResidentText& r : c->resident) {
        (void)hipFree(r.dev);
        (void)hipFree(r.tile_off);
    }
    c->resident.clear();
    for (void* hp : c->host_blocks) (void)hipHostFree(hp);
    if (c->host_back) (void)hipHostFree(c->host_back);
    for (const wk_ctx::HostReg& r : c->regs) (void)hipHostUnregister(const_cast<char*>(r.p));
    c->regs.clear();
    if (c->di_any_host) (void)hipHostFree(c->di_any_host);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->count_stream) (void)hipStreamDestroy(c->count_stream);
    if (c->res_ev) (void)hipEventDestroy(c->res_ev);
    for (hipEvent_t ev : c->slot_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (DevBuf& b : c->rank_tab) b.release();
    for (auto& kv : c->ktimers)
        if (kv.second.b) (void)hipEventDestroy(kv.second.b);
    if (c->kt_step) (void)hipEventDestroy(c->kt_step);
    if (c->t0) (void)hipEventDestroy(c->t0);
    if (c->t1) (void)hipEventDestroy(c->t1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int wk_device_name(const wk_ctx* c, char* buf, size_t cap) {
    if (!c || !buf || cap == 0) return WK_E_ARG;
    snprintf(buf, cap, "%s (%s, %d CUs)", c->prop.name, c->prop.gcnArchName, c->prop.multiProcessorCount);
    return WK_OK;
}

int wk_sync(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->count_stream) HIP_TRY(c, hipStreamSynchronize(c->count_stream));  // (newline counts behind copies / resident blocks)
    return WK_OK;
}

int wk_set_option(wk_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return WK_E_ARG;
    if (!strcmp(name, "gene_index_pairs")) {  // the next wk_set_genes: gene lists by gene table index (wk_ordinal_pair_genes)
        c->gene_index_opt = value != 0;
        return WK_OK;
    }
    if (!strcmp(name, "dtok_count_ahead")) {  // 0: no newline count behind the copies of blocks (wk_dtok_copy*): the scans count the blocks that need it
        c->count_ahead = value != 0;
        return WK_OK;
    }
    if (!strcmp(name, "cover_cap_rows")) {  // rows of the coverage pile that wk_cover_begin(ctx, 0) reserves (0: the default); results never depend on it
        if (value != 0 && (value < kCoverCapMin || value > kCoverCapMax))
            return fail(c, WK_E_ARG, "cover_cap_rows must be 0 or in [%lld, %lld]", (long long)kCoverCapMin, (long long)kCoverCapMax);
        c->cv_cap_opt = value;
        return WK_OK;
    }
    if (!strcmp(name, "demux_hash_mask")) {  // (tests) AND-ed into every hash of a sample name, 0: none; before wk_demux_begin
        c->dx_hash_mask = (uint64_t)value;
        return WK_OK;
    }
    if (!strcmp(name, "demux_max_samples")) {  // (tests) samples the table takes, 0: kDemuxMaxSamples; before wk_demux_begin
        if (value < 0 || value > (int64_t)kDemuxMaxSamples) return fail(c, WK_E_ARG, "demux_max_samples must be in [0, %u]", kDemuxMaxSamples);
        c->dx_max_opt = value;
        return WK_OK;
    }
    if (!strcmp(name, "readmap_demux_cap")) {  // entries (tiles x samples of a block) of the matrix the read maps under demultiplexing are partitioned with, 0: the default; a block beyond it is the host's
        if (value < 0 || value > kPartCapMax) return fail(c, WK_E_ARG, "readmap_demux_cap must be in [0, %lld]", (long long)kPartCapMax);
        c->pd_cap_opt = value;
        return WK_OK;
    }
    return fail(c, WK_E_ARG, "unknown option '%s' (launch shapes and ablation switches: wk_tune)", name);
}

// Launch shapes, ablation switches and what bench.py needs to time repeated passes:
// measurement only — nothing in woltka_amd/ calls it, results never depend on it.
int wk_tune(wk_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return WK_E_ARG;
    if (!strcmp(name, "lds_slots")) {
        if (value < 64 || value > 8192 || (value & (value - 1))) return fail(c, WK_E_ARG, "lds_slots must be a power of two in [64, 8192]");
        c->lds_slots = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "blocks_per_cu")) {
        if (value < 1 || value > 32) return fail(c, WK_E_ARG, "blocks_per_cu must be in [1, 32]");
        c->blocks_per_cu = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "threads")) {
        if (value < 64 || value > 1024 || (value % 64)) return fail(c, WK_E_ARG, "threads must be a multiple of 64 in [64, 1024]");
        c->threads = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "ablate")) {
        c->ablate = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "free_sparse")) {  // 0: `--rank free` walks up the tree per read
        c->use_free_sparse = (int)value;
        c->rows_sig.clear();
        return WK_OK;
    }
    if (!strcmp(name, "tally_per_cu")) {
        if (value < 1 || value > 4) return fail(c, WK_E_ARG, "tally_per_cu must be in [1, 4]");
        c->tally_per_cu = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "tally_slots")) {
        if (value < 256 || value > 4096 || (value & (value - 1))) return fail(c, WK_E_ARG, "tally_slots must be a power of two in [256, 4096]");
        c->tally_slots = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "dtok_fused")) {
        if (value != 0 && value != 1) return fail(c, WK_E_ARG, "dtok_fused must be 0 or 1");
        c->use_fused = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "fz_ablate")) {
        c->fused_ablate = (uint32_t)value;
        return WK_OK;
    }
    if (!strcmp(name, "dtok_fused_per_cu")) {
        if (value < 1 || value > 8) return fail(c, WK_E_ARG, "dtok_fused_per_cu must be in [1, 8]");
        c->fused_per_cu = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "stripes_min")) {
        if (value < 0) return fail(c, WK_E_ARG, "stripes_min must be >= 0");
        c->stripes_min_hits = value;
        return WK_OK;
    }
    if (!strcmp(name, "stripes")) {
        if (value != 0 && value != 1) return fail(c, WK_E_ARG, "stripes must be 0 or 1");
        c->use_stripes = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "tally")) {
        c->use_tally = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "match_lds")) {
        c->match_lds = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "grid_density")) {  // takes effect at the next wk_set_genes
        if (value < 1 || value > 8) return fail(c, WK_E_ARG, "grid_density must be in [1, 8]");
        c->grid_density = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "plog")) {  // 0 = off, 1 = auto (large chunks), 2 = always
        c->use_plog = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "log_parts")) {  // 0 = auto, 256 or 1024
        if (value != 0 && (value < 64 || value > 1024 || (value & (value - 1)))) return fail(c, WK_E_ARG, "log_parts must be 0 or a power of two in [64, 1024]");
        c->log_parts_opt = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "plog_max_bytes")) {
        if (value < (1 << 20)) return fail(c, WK_E_ARG, "plog_max_bytes must be at least 1 MiB");
        c->plog_max_bytes = value;
        return WK_OK;
    }
    if (!strcmp(name, "dense")) {
        c->use_dense = value ? 1 : 0;
        return WK_OK;
    }
    if (!strcmp(name, "split")) {  // 0 = off, 1 = auto, 2 = always (when the chunk qualifies)
        if (value < 0 || value > 2) return fail(c, WK_E_ARG, "split must be 0, 1 or 2");
        c->use_split = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "hot_bins")) {
        c->use_hot_bins = value ? 1 : 0;
        return WK_OK;
    }
    if (!strcmp(name, "subject_bins")) {
        c->use_subject_bins = value ? 1 : 0;
        return WK_OK;
    }
    if (!strcmp(name, "count_kernel")) {
        c->use_count_kernel = value ? 1 : 0;
        return WK_OK;
    }
    if (!strcmp(name, "single_blocks_per_cu")) {
        if (value < 1 || value > 8) return fail(c, WK_E_ARG, "single_blocks_per_cu must be in [1, 8]");
        c->single_blocks_per_cu = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "lap_print")) {
        fprintf(stderr, "[wk] seconds inside wk_dtok_copy %.3f, wk_dtok_scan(_emit) %.3f of which waiting for the stream %.3f, for the copy %.3f\n", c->lap_s[0],
                c->lap_s[1], c->lap_s[2], c->lap_s[3]);
        fprintf(stderr, "[wk] copy calls, host side: streams + events %.3f, device buffer %.3f (longest %.3f), copy queued %.3f, count queued %.3f\n", c->lap_c[0],
                c->lap_c[1], c->lap_c[4], c->lap_c[2], c->lap_c[3]);
        for (double& x : c->lap_c) x = 0;
        if (c->lap_copy_ms > 0)
            fprintf(stderr, "[wk] the copies themselves: %.1f ms for %.2f GB = %.1f GB/s (events around each copy + newline count on the copy stream)\n",
                    c->lap_copy_ms, (double)c->lap_copy_bytes / 1e9, (double)c->lap_copy_bytes / 1e6 / c->lap_copy_ms);
        fprintf(stderr, "[wk] scan, host side: claim %.3f, line starts queued %.3f, parse queued %.3f, emission queued %.3f, finish %.3f, names %.3f\n",
                c->lap_x[0], c->lap_x[1], c->lap_x[2], c->lap_x[3], c->lap_x[4], c->lap_x[5]);
        for (double& x : c->lap_x) x = 0;
        c->lap_s[0] = c->lap_s[1] = c->lap_s[2] = c->lap_s[3] = 0;
        c->lap_copy_ms = 0;
        c->lap_copy_bytes = 0;
        return WK_OK;
    }
    if (!strcmp(name, "range_parts")) {  // partitions of the dense gene log (a power of two; 0 = auto)
        c->range_parts_opt = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "streams")) {  // 0: the records of all slices in one stream (round 3's team kernel)
        c->use_streams = value != 0;
        return WK_OK;
    }
    if (!strcmp(name, "weigh")) {  // 0 = off, 1 = auto (large multi-hit chunks), 2 = whenever the jobs allow it
        if (value < 0 || value > 2) return fail(c, WK_E_ARG, "weigh must be 0, 1 or 2");
        c->use_weigh = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "free_per_cu")) {
        if (value < 1 || value > 8) return fail(c, WK_E_ARG, "free_per_cu must be in [1, 8]");
        c->free_per_cu = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "range_log")) {
        c->use_range_log = value != 0;
        return WK_OK;
    }
    if (!strcmp(name, "free_threads")) {
        if (value != 256 && value != 512 && value != 1024) return fail(c, WK_E_ARG, "free_threads must be 256, 512 or 1024");
        c->free_threads = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "free_slots")) {
        if (value < 256 || value > 8192 || (value & (value - 1))) return fail(c, WK_E_ARG, "free_slots must be a power of two in [256, 8192]");
        c->free_slots = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "words_keep")) {
        c->words_keep = value ? 1 : 0;
        return WK_OK;
    }
    if (!strcmp(name, "weigh_wide")) {
        if (value != 0 && value != 1) return fail(c, WK_E_ARG, "weigh_wide must be 0 or 1");
        c->weigh_wide = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "weigh_wide_wgs")) {
        if (value < 0 || value > (int64_t)kWideMaxWgs) return fail(c, WK_E_ARG, "weigh_wide_wgs must be in [0, %u]", kWideMaxWgs);
        c->weigh_wide_wgs = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "bins_ring")) {
        c->bins_ring = (int)value;
        return WK_OK;
    }
    if (!strcmp(name, "tiled")) {
        c->tiled = value ? 1 : 0;
        return WK_OK;
    }
    if (!strcmp(name, "use_lds")) {
        c->use_lds = value ? 1 : 0;
        return WK_OK;
    }
    return fail(c, WK_E_ARG, "unknown tuning knob '%s'", name);
}

// ---- static state ----------------------------------------------------------

int wk_set_tree(wk_ctx* c, const int32_t* parent, const int32_t* last, const int32_t* rank_code, int32_t n) {
    if (!c) return WK_E_ARG;
    if (n < 0 || (n > 0 && (!parent || !last || !rank_code))) return fail(c, WK_E_ARG, "bad tree arguments");
    if ((int64_t)n > (int64_t)WK_MAX_FEATURE) return fail(c, WK_E_RANGE, "too many hierarchy nodes");
    DeviceGuard guard(c->device);
    {
        const int rcw = wk_words_flush(c);  // (records accumulated under the old tree)
        if (rcw) return rcw;
    }
    for (int32_t v = 0; v < n; ++v) {  // validate the pre-order contract the kernels rely on
        const bool ok = (v == 0) ? (parent[0] == 0) : (parent[v] >= 0 && parent[v] < v);
        if (!ok || last[v] < v || last[v] >= n) return fail(c, WK_E_ARG, "node %d violates the pre-order contract (parent %d, last %d)", v, parent[v], last[v]);
    }
    std::vector<Node> packed((size_t)n);
    for (int32_t v = 0; v < n; ++v) packed[v] = Node{parent[v], last[v]};
    int rc;
    if ((rc = upload(c, c->nodes, packed.data(), (size_t)n * sizeof(Node)))) return rc;
    if ((rc = upload(c, c->rank_code, rank_code, (size_t)n * sizeof(int32_t)))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // `packed` is about to go out of scope
    c->rank_code_host.assign(rank_code, rank_code + n);
    c->parent_host.assign(parent, parent + n);
    c->last_host.assign(last, last + n);
    c->tree_serial += 1;
    c->n_nodes = n;
    c->rows_sig.clear();
    for (bool& v : c->rank_tab_valid) v = false;
    return WK_OK;
}

int wk_build_rank_table(wk_ctx* c, int32_t slot, int32_t code) {
    if (!c) return WK_E_ARG;
    if (slot < 0 || slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0])) return fail(c, WK_E_ARG, "rank slot %d out of range", slot);
    if (c->n_nodes <= 0) return fail(c, WK_E_STATE, "no hierarchy uploaded (wk_set_tree)");
    DeviceGuard guard(c->device);
    HIP_TRY(c, c->rank_tab[slot].reserve((size_t)c->n_nodes * sizeof(int32_t)));
    KernelTimer* kt = ktimer_begin(c, "rank_table");
    hipLaunchKernelGGL(rank_table_kernel, dim3((c->n_nodes + 255) / 256), dim3(256), 0, c->stream,
                       c->nodes.as<Node>(), c->rank_code.as<int32_t>(), c->n_nodes, code,
                       c->rank_tab[slot].as<int32_t>());
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    c->rank_tab_valid[slot] = true;
    c->rank_tab_code[slot] = code;
    c->rank_serial += 1;
    c->rank_tab_nodes[slot] = std::count(c->rank_code_host.begin(), c->rank_code_host.end(), code);
    c->rows_sig.clear();
    return WK_OK;
}

int wk_get_rank_table(wk_ctx* c, int32_t slot, int32_t* out) {
    if (!c || !out) return WK_E_ARG;
    if (slot < 0 || slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) || !c->rank_tab_valid[slot])
        return fail(c, WK_E_STATE, "rank slot %d has not been built", slot);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(out, c->rank_tab[slot].p, (size_t)c->n_nodes * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

int wk_set_genes(wk_ctx* c, const int32_t* genome_off, int32_t n_genomes, const int32_t* start0,
                 const int32_t* end, const int32_t* gene_feature, int32_t n_genes) {
    if (!c) return WK_E_ARG;
    if (n_genomes < 0 || n_genes < 0 || !genome_off || (n_genes > 0 && (!start0 || !end || !gene_feature)))
        return fail(c, WK_E_ARG, "bad gene table arguments");
    if (genome_off[0] != 0 || genome_off[n_genomes] != n_genes) return fail(c, WK_E_ARG, "genome_off must run from 0 to n_genes");
    // gene records {start0, end, largest end before the gene, feature}: the
    // third word stops the backward walk of a hit
    std::vector<int32_t> packed((size_t)n_genes * 4);
    for (int32_t g = 0; g < n_genomes; ++g) {
        if (genome_off[g + 1] < genome_off[g]) return fail(c, WK_E_ARG, "genome_off is not monotone at genome %d", g);
        int32_t m = INT32_MIN;
        for (int32_t i = genome_off[g]; i < genome_off[g + 1]; ++i) {
            if (i > genome_off[g] && start0[i] < start0[i - 1]) return fail(c, WK_E_ARG, "genes of genome %d are not sorted by start", g);
            if (end[i] < start0[i]) return fail(c, WK_E_ARG, "gene %d has end < start", i);
            if (gene_feature[i] < 0 || gene_feature[i] > WK_MAX_FEATURE) return fail(c, WK_E_RANGE, "gene feature id out of range");
            packed[4 * (size_t)i] = start0[i];
            packed[4 * (size_t)i + 1] = end[i];
            packed[4 * (size_t)i + 2] = m;
            packed[4 * (size_t)i + 3] = c->gene_index_opt ? i : gene_feature[i];
            m = end[i] > m ? end[i] : m;
        }
    }
    // grid per genome: `cells` (a power of two, about grid_density per gene)
    // equal ranges of width 2^shift from the smallest start0 on;
    // grid[off + c] = first gene whose cell is >= c, for c = 0 .. cells
    std::vector<int32_t> first((size_t)n_genomes + 1, 0), goff((size_t)n_genomes + 1, 0);
    std::vector<unsigned char> shift((size_t)n_genomes + 1, 0);
    std::vector<int32_t> grid;
    grid.reserve((size_t)n_genes * 2 * (size_t)c->grid_density + (size_t)n_genomes * 2 + 1);
    for (int32_t g = 0; g < n_genomes; ++g) {
        const int32_t lo = genome_off[g], n = genome_off[g + 1] - lo;
        goff[g] = (int32_t)grid.size();
        if (n == 0) continue;  // no cells: no hit of this genome matches
        first[g] = start0[lo];
        const uint64_t span = (uint64_t)((int64_t)start0[lo + n - 1] - (int64_t)start0[lo]);
        uint64_t cells = 1;
        while (cells < (uint64_t)n * (uint64_t)c->grid_density) cells <<= 1;
        int sh = 0;
        while ((span >> sh) >= cells) sh += 1;
        shift[g] = (unsigned char)sh;
        if (grid.size() + cells + 1 >= (1ull << 31)) return fail(c, WK_E_RANGE, "gene tables too large for the coordinate grid");
        int32_t i = lo;
        for (uint64_t cell = 0; cell <= cells; ++cell) {
            while (i < lo + n && (((uint64_t)((int64_t)start0[i] - (int64_t)start0[lo])) >> sh) < cell) i += 1;
            grid.push_back(i);
        }
    }
    goff[n_genomes] = (int32_t)grid.size();
    if (grid.empty()) grid.push_back(0);
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = upload(c, c->gene4, packed.data(), packed.size() * sizeof(int32_t)))) return rc;
    if ((rc = upload(c, c->g_grid, grid.data(), grid.size() * sizeof(int32_t)))) return rc;
    if ((rc = upload(c, c->g_first, first.data(), first.size() * sizeof(int32_t)))) return rc;
    if ((rc = upload(c, c->g_goff, goff.data(), goff.size() * sizeof(int32_t)))) return rc;
    if ((rc = upload(c, c->g_shift, shift.data(), shift.size()))) return rc;
    if ((rc = upload(c, c->g_feature, gene_feature, (size_t)n_genes * 4))) return rc;
    // genome stripes for the sorted coord-match (wk_stripe.hpp): consecutive genomes while their genes, the
    // cells of their grids and their per-genome words fit the LDS; a genome that does not fit alone has no
    // stripe (its hits keep the gather kernels)
    {
        std::vector<int32_t> stripe_of((size_t)std::max(n_genomes, 1), -1);
        c->stripes_host.clear();
        auto genes_of = [&](int32_t g) { return genome_off[g + 1] - genome_off[g]; };
        auto cells_of = [&](int32_t g) { return goff[g + 1] - goff[g]; };
        int32_t g = 0;
        while (g < n_genomes) {
            if ((uint32_t)genes_of(g) > kStripeGenes || (uint32_t)cells_of(g) > kStripeCells) {
                ++g;
                continue;
            }
            StripeInfo si{};
            si.gene_lo = genome_off[g];
            si.genome_lo = g;
            si.cell_lo = goff[g];
            const int32_t sid = (int32_t)c->stripes_host.size();
            while (g < n_genomes && (uint32_t)(si.n_genes + genes_of(g)) <= kStripeGenes && (uint32_t)(si.n_cells + cells_of(g)) <= kStripeCells &&
                   (uint32_t)si.n_genomes < kStripeGenomes) {
                si.n_genes += genes_of(g);
                si.n_cells += cells_of(g);
                si.n_genomes += 1;
                stripe_of[g] = sid;
                ++g;
            }
            c->stripes_host.push_back(si);
        }
        c->stripes_usable = !c->stripes_host.empty() && n_genes > 0;
        if (c->stripes_host.empty()) c->stripes_host.push_back(StripeInfo{});
        if ((rc = upload(c, c->g_stripe_of, stripe_of.data(), stripe_of.size() * 4))) return rc;
        if ((rc = upload(c, c->g_stripes, c->stripes_host.data(), c->stripes_host.size() * sizeof(StripeInfo)))) return rc;
        if ((rc = upload(c, c->g_gene_off, genome_off, ((size_t)n_genomes + 1) * 4))) return rc;
    }
    c->genes_by_index = c->gene_index_opt != 0;
    c->genes_set = true;
    c->sb_valid = false;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->n_genomes = n_genomes;
    c->n_genes = n_genes;
    c->max_gene_feature = 0;
    for (int32_t i = 0; i < n_genes; ++i) c->max_gene_feature = std::max(c->max_gene_feature, gene_feature[i]);
    return WK_OK;
}

int wk_set_subjects(wk_ctx* c, const int32_t* feature_of_subject, int32_t n) {
    if (!c) return WK_E_ARG;
    if (n < 0 || (n > 0 && !feature_of_subject)) return fail(c, WK_E_ARG, "bad subject table arguments");
    int32_t mx = -1;
    for (int32_t s = 0; s < n; ++s) {
        if (feature_of_subject[s] < 0 || feature_of_subject[s] > WK_MAX_FEATURE)
            return fail(c, WK_E_RANGE, "subject %d: feature id outside [0, %d]", s, WK_MAX_FEATURE);
        mx = std::max(mx, feature_of_subject[s]);
    }
    c->max_subject_feature = mx;
    DeviceGuard guard(c->device);
    int rc;
    // accumulated packed records name subjects of the old table: they stay
    // valid only if the new table extends it
    if (c->w_open && c->w_records > 0 &&
        (n < c->n_subjects || memcmp(feature_of_subject, c->subj_feat_host.data(), (size_t)c->n_subjects * 4) != 0) &&
        (rc = wk_words_flush(c)))
        return rc;
    rc = upload(c, c->subj_feat, feature_of_subject, (size_t)n * sizeof(int32_t));
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->n_subjects = n;
    c->subj_feat_host.assign(feature_of_subject, feature_of_subject + n);
    c->subj_serial += 1;
    c->rows_sig.clear();  // rows are rebuilt on the next classify call
    return WK_OK;
}

// ---- count table -------------------------------------------------------------

int wk_counts_clear(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    if (!c->slots) return fail(c, WK_E_STATE, "count table not reserved");
    DeviceGuard guard(c->device);
    if (!c->words_keep) {  // accumulated records are counts that have not been added yet
        c->w_records = c->w_reads = 0;
        c->w_open = false;
    }
    HIP_TRY(c, hipMemsetAsync(c->tkeys.p, 0xFF, c->slots * sizeof(uint64_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->tvals.p, 0, c->slots * sizeof(uint64_t), c->stream));
    return WK_OK;
}

int wk_counts_reserve(wk_ctx* c, int64_t min_slots) {
    if (!c) return WK_E_ARG;
    if (min_slots < 1) min_slots = 1;
    uint64_t s = 1024;
    while (s < (uint64_t)min_slots) s <<= 1;
    DeviceGuard guard(c->device);
    if (s != c->slots) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->tkeys.release();
        c->tvals.release();
        HIP_TRY(c, c->tkeys.reserve(s * sizeof(uint64_t)));
        HIP_TRY(c, c->tvals.reserve(s * sizeof(uint64_t)));
        c->slots = s;
    }
    return wk_counts_clear(c);
}

int wk_counts_fetch(wk_ctx* c, uint64_t* keys, int64_t* counts, int64_t cap, int64_t* n) {
    if (!c || !n) return WK_E_ARG;
    if (!c->slots) return fail(c, WK_E_STATE, "count table not reserved");
    DeviceGuard guard(c->device);
    int rc = c->words_keep ? WK_OK : wk_words_flush(c);  // records still accumulated (wk_words_append) are counted now
    if (rc) return rc;
    if ((rc = check_device_errors(c))) return rc;
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 4), 0, sizeof(unsigned long long), c->stream));
    const int blocks = grid_for((int64_t)c->slots, 256, 2048);
    hipLaunchKernelGGL(table_count_kernel, dim3(blocks), dim3(256), 0, c->stream, c->tkeys.as<unsigned long long>(),
                       c->slots, scalar_u64(c, 4));
    HIP_TRY(c, hipGetLastError());
    unsigned long long used = 0;
    HIP_TRY(c, hipMemcpyAsync(&used, scalar_u64(c, 4), sizeof used, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n = (int64_t)used;
    if ((int64_t)used > cap || (used && (!keys || !counts))) return fail(c, WK_E_CAPACITY, "output capacity %lld < %llu entries", (long long)cap, used);
    if (used == 0) return WK_OK;
    HIP_TRY(c, c->fetch_k.reserve(used * sizeof(uint64_t)));
    HIP_TRY(c, c->fetch_v.reserve(used * sizeof(int64_t)));
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 4), 0, sizeof(unsigned long long), c->stream));
    KernelTimer* kt = ktimer_begin(c, "compact");
    hipLaunchKernelGGL(table_compact_kernel, dim3(blocks), dim3(256), 0, c->stream, c->tkeys.as<unsigned long long>(),
                       c->tvals.as<unsigned long long>(), c->slots, scalar_u64(c, 4),
                       c->fetch_k.as<unsigned long long>(), c->fetch_v.as<long long>());
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(keys, c->fetch_k.p, used * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts, c->fetch_v.p, used * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

int wk_log_reserve(wk_ctx* c, int64_t n_entries) {
    if (!c) return WK_E_ARG;
    if (n_entries < 1) return fail(c, WK_E_ARG, "log capacity must be positive");
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, c->log.reserve((size_t)n_entries * 16));
    c->log_cap = n_entries;
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 5), 0, 8, c->stream));
    return WK_OK;
}

int wk_log_fetch(wk_ctx* c, int32_t* out, int64_t cap, int64_t* n) {
    if (!c || !n) return WK_E_ARG;
    DeviceGuard guard(c->device);
    int rc = check_device_errors(c);
    if (rc) return rc;
    unsigned long long used = 0;
    HIP_TRY(c, hipMemcpyAsync(&used, scalar_u64(c, 5), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n = (int64_t)used;
    if ((int64_t)used > c->log_cap) {
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 5), 0, 8, c->stream));
        return fail(c, WK_E_CAPACITY, "contribution log overflowed: %llu entries needed, %lld reserved", used, (long long)c->log_cap);
    }
    if ((int64_t)used > cap || (used && !out)) return fail(c, WK_E_CAPACITY, "output capacity %lld < %llu entries", (long long)cap, used);
    if (used) HIP_TRY(c, hipMemcpyAsync(out, c->log.p, (size_t)used * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 5), 0, 8, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// ---- classify ----------------------------------------------------------------

int wk_chunk_stage(wk_ctx* c, const int32_t* subj, const int32_t* qoff, int64_t n_reads, const int32_t* group,
                   int subj_flags) {
    if (!c) return WK_E_ARG;
    if (n_reads < 0 || !qoff) return fail(c, WK_E_ARG, "bad chunk arguments");
    const int64_t n_rec = qoff[n_reads];
    if (qoff[0] != 0 || n_rec < 0 || (n_rec > 0 && !subj)) return fail(c, WK_E_ARG, "qoff must start at 0 and end at n_records");
    const bool uniform = (subj_flags & WK_GROUP_UNIFORM) != 0;
    if (uniform && (!group || group[0] < 0 || group[0] >= (1 << WK_KEY_GROUP_BITS)))
        return fail(c, WK_E_ARG, "WK_GROUP_UNIFORM needs one group id in [0, %d)", 1 << WK_KEY_GROUP_BITS);
    DeviceGuard guard(c->device);
    int rc;
    // (64 bytes of slack behind the records: the weighted histogram reads them 16 bytes at a time)
    HIP_TRY(c, c->c_subj.reserve((size_t)n_rec * sizeof(int32_t) + 64));
    if ((rc = upload(c, c->c_subj, subj, (size_t)n_rec * sizeof(int32_t)))) return rc;
    if ((rc = upload(c, c->c_qoff, qoff, ((size_t)n_reads + 1) * sizeof(int32_t)))) return rc;
    if (group && !uniform && (rc = upload(c, c->c_group, group, (size_t)n_reads * sizeof(int32_t)))) return rc;
    // the read size of every record (what the record histogram of wk_weigh.hpp
    // streams next to the subject indices) + the reads it does not cover
    c->rk_valid[0] = c->rk_valid[1] = false;
    c->stage_serial += 1;
    unsigned long long totals[2] = {0, 0};
    if (c->use_weigh && (subj_flags & WK_SUBJ_INDEXED) && (subj_flags & WK_SUBJ_IS_SET) && n_reads > 0 &&
        n_reads < (1ll << 30) && n_rec < (1ll << 30)) {
        HIP_TRY(c, c->c_rk[0].reserve((size_t)n_rec + 64));
        HIP_TRY(c, c->rk_left[0].reserve((size_t)((n_reads + 63) / 64) * 8));
        HIP_TRY(c, c->rk_totals.reserve(32));
        KernelTimer* kt = ktimer_begin(c, "read_sizes");
        if ((rc = derive_read_sizes(c, false, c->c_qoff.as<int32_t>(), c->c_subj.as<int32_t>(), n_reads, n_rec,
                                    c->c_rk[0].as<unsigned char>(), c->rk_left[0].as<unsigned long long>(),
                                    c->rk_totals.as<unsigned long long>())))
            return rc;
        ktimer_end(c, kt);
        HIP_TRY(c, hipMemcpyAsync(totals, c->rk_totals.p, 16, hipMemcpyDeviceToHost, c->stream));
        c->rk_valid[0] = true;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // host buffers are only valid during the call
    c->rk_reads[0] = (int64_t)totals[0];
    c->rk_records[0] = (int64_t)totals[1];
    c->cur_subj = c->c_subj.as<int32_t>();
    c->cur_qoff = c->c_qoff.as<int32_t>();
    c->n_reads = n_reads;
    c->n_records = n_rec;
    c->has_group = group != nullptr && !uniform;
    c->dx_hits = false;
    c->group_base = uniform ? group[0] : 0;
    c->subj_is_set = (subj_flags & WK_SUBJ_IS_SET) != 0;
    c->subj_indexed = (subj_flags & WK_SUBJ_INDEXED) != 0;
    c->chunk_valid = true;
    c->dx_chunk = false;
    c->rr_chunk = false;
    c->rd_chunk = false;
    return WK_OK;
}

static int classify_staged_impl(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t* out_assign, bool keep);

int wk_classify_staged(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t* out_assign) {
    return classify_staged_impl(c, jobs, n_jobs, out_assign, false);
}

// The same with the codes left where classify_kernel writes them (assign_out, job-major) and nothing copied to
// the host: wk_dtok_readmap_reads formats the read maps from them.
int wk_classify_staged_keep(wk_ctx* c, const wk_job* jobs, int32_t n_jobs) {
    const int rc = classify_staged_impl(c, jobs, n_jobs, nullptr, true);
    if (rc) return rc;
    c->rr_serial = c->stage_serial;
    c->rr_jobs = n_jobs;
    c->rr_unassigned = (jobs[0].flags & WK_F_UNASSIGNED) ? 1u : 0u;
    for (int j = 0; j < n_jobs; ++j) {
        c->rl_mode[j] = jobs[j].mode;
        c->rl_slot[j] = jobs[j].rank_slot;
    }
    return WK_OK;
}

// `keep`: the codes are written as for `out_assign` and stay on the device.
static int classify_staged_impl(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t* out_assign, bool keep) {
    if (!c) return WK_E_ARG;
    c->rr_serial = -1;  // (whatever assign_out held is overwritten or stale from here on)
    const bool want_codes = out_assign != nullptr || keep;
    if (!jobs || n_jobs < 1 || n_jobs > WK_MAX_JOBS) return fail(c, WK_E_ARG, "n_jobs must be in [1,%d]", WK_MAX_JOBS);
    if (!c->chunk_valid) return fail(c, WK_E_STATE, "no chunk staged");
    if (!c->slots) return fail(c, WK_E_STATE, "count table not reserved (wk_counts_reserve)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);

    ClassifyArgs a{};
    a.subj = c->cur_subj;
    a.qoff = c->cur_qoff;
    a.group = c->has_group ? c->c_group.as<int32_t>() : nullptr;
    a.group_base = c->has_group ? 0 : c->group_base;
    a.n_reads = c->n_reads;
    a.nodes = c->n_nodes ? c->nodes.as<Node>() : nullptr;
    a.n_nodes = c->n_nodes;
    a.n_jobs = n_jobs;
    a.subj_is_set = c->subj_is_set ? 1 : 0;
    for (int j = 0; j < n_jobs; ++j) {
        const wk_job& jb = jobs[j];
        JobDev d{};
        d.mode = jb.mode;
        d.flags = jb.flags;
        d.major = jb.major;
        d.anc = nullptr;
        if (jb.mode == WK_MODE_FREE || jb.mode == WK_MODE_RANK) {
            if (c->n_nodes <= 0) return fail(c, WK_E_STATE, "job %d needs a hierarchy (wk_set_tree)", j);
        } else if (jb.mode != WK_MODE_NONE) {
            return fail(c, WK_E_ARG, "job %d: unknown mode %d", j, jb.mode);
        }
        if (jb.mode == WK_MODE_RANK) {
            if (jb.rank_slot < 0 || jb.rank_slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) || !c->rank_tab_valid[jb.rank_slot])
                return fail(c, WK_E_STATE, "job %d: rank slot %d has not been built", j, jb.rank_slot);
            d.anc = c->rank_tab[jb.rank_slot].as<int32_t>();
            if (jb.major < 0.0 || jb.major > 1.0) return fail(c, WK_E_ARG, "job %d: major must be a fraction in [0,1]", j);
        }
        a.jobs[j] = d;
    }
    if (c->subj_indexed) {
        const int rc_rows = build_subject_rows(c, jobs, n_jobs, a);
        if (rc_rows) return rc_rows;
    } else {
        // chunk of feature ids: rank columns for the first pass of the split
        // (at most three distinct ranks, like a subject row)
        int slots[3];
        int n_cols = 0;
        for (int j = 0; j < n_jobs && n_cols >= 0; ++j) {
            if (jobs[j].mode != WK_MODE_RANK) continue;
            int col = -1;
            for (int q = 0; q < n_cols; ++q)
                if (slots[q] == jobs[j].rank_slot) col = q;
            if (col < 0) {
                if (n_cols == 3) {
                    n_cols = -1;  // too many ranks: no split for this launch
                    break;
                }
                col = n_cols++;
                slots[col] = jobs[j].rank_slot;
                a.col_anc[col] = c->rank_tab[jobs[j].rank_slot].as<int32_t>();
            }
            a.jobs[j].col = col;
        }
        a.n_cols = n_cols;
    }
    if (want_codes) {
        HIP_TRY(c, c->assign_out.reserve((size_t)n_jobs * (size_t)(c->n_reads ? c->n_reads : 1) * sizeof(int32_t)));
        a.out_assign = c->assign_out.as<int32_t>();
    }
    a.stat_block = c->stat_block.as<unsigned long long>();
    a.ablate = (uint32_t)c->ablate;
    a.log = c->log.as<int32_t>();
    a.log_cursor = scalar_u64(c, 5);
    a.log_cap = c->log_cap;
    for (int j = 0; j < n_jobs; ++j)
        if ((jobs[j].flags & WK_F_SIZED) && c->log_cap <= 0)
            return fail(c, WK_E_STATE, "job %d is size-normalised but no log is reserved (wk_log_reserve)", j);
    a.table = CountTable{c->tkeys.as<unsigned long long>(), c->tvals.as<unsigned long long>(), c->slots - 1, scalar_err(c)};

    if (c->n_reads > 0) {
        KernelTimer* kt = ktimer_begin(c, "classify");
        if (c->use_lds && c->tiled && !c->subj_indexed) {
            // persistent workgroups, each with its own tile buffers + LDS front cache
            const size_t lds = (size_t)(kTileWindow + 4 + kTileReads + 4) * sizeof(int32_t) + (size_t)c->lds_slots * 16;
            const int64_t n_tiles = (c->n_reads + kTileReads - 1) / kTileReads;
            const int blocks = (int)std::min<int64_t>(std::min<int64_t>(n_tiles, kStatBlocks), (int64_t)c->prop.multiProcessorCount * c->blocks_per_cu);
            hipLaunchKernelGGL(classify_tiled_kernel, dim3(blocks), dim3(kTileThreads), lds, c->stream, a,
                               (uint32_t)c->lds_slots, c->n_records);
        } else if (c->use_lds) {
            bool sized = false;
            for (int j = 0; j < n_jobs; ++j) sized |= (jobs[j].flags & WK_F_SIZED) != 0;
            // two-class split (32-bit byte offsets in the first pass bound the
            // sizes).  It pays even when only half of the reads have a single
            // candidate (config 3: 10.6 -> 7.7 ms); a chunk without any pays one
            // streaming pass over the offsets.
            const bool feature_chunk = !c->subj_indexed;
            // (ext: the caller evaluates only the reads of its own bit mask — wk_ordinal_count's leftovers)
            const bool ext = c->listed_only;
            const bool split = !ext && c->use_split && c->n_reads < (1ll << 30) && c->n_records < (1ll << 30) &&
                               (feature_chunk ? a.n_cols >= 0 : (a.row_w == 4 && c->n_subjects < (1 << 28)));
            // ... and with a small subject table the first pass only histograms
            // subject indices; the assigners run once per subject afterwards
            const bool subject_ok = split && !feature_chunk && c->use_subject_bins && !want_codes && !c->has_group && !sized;
            const bool by_subject = subject_ok && c->n_subjects <= 28672;
            // a larger table: the first 24,576 subject indices (first appearance
            // order: the abundant ones) in bins, the others per read
            const bool hot_subjects = subject_ok && !by_subject && c->use_subject_bins >= 1 && c->use_hot_bins;
            constexpr int kHotBins = 24576;
            // weighted subject histogram (wk_weigh.hpp): plain assigners only, every
            // read a set of subject indices, one group, no per-read output
            bool weigh = !ext && c->use_weigh && c->subj_indexed && c->subj_is_set && !c->has_group && !want_codes && !sized &&
                         c->n_reads < (1ll << 30) && c->n_records < (1ll << 30) && c->n_subjects > 0;
            for (int j = 0; j < n_jobs && weigh; ++j) {
                if (jobs[j].mode == WK_MODE_NONE)
                    weigh = !(jobs[j].flags & WK_F_UNIQ);
                else if (jobs[j].mode == WK_MODE_RANK)
                    weigh = !(jobs[j].flags & (WK_F_UNIQ | WK_F_ABOVE)) && !(jobs[j].major > 0.0);
                else
                    weigh = false;
            }
            // auto: chunks that are worth the fixed cost (slab rows of every
            // workgroup) and are not all single-candidate reads (the count-first
            // pass above is the faster special case of those)
            if (weigh && c->use_weigh == 1)
                weigh = c->n_reads >= (1 << 16) && c->n_records > c->n_reads + c->n_reads / 64;
            uint32_t w_bins = 0, w_slices = 0, w_teams = 0, w_xcd = 8;
            weigh = weigh && c->rk_valid[0] && a.subj == c->c_subj.as<int32_t>();
            if (weigh) {
                const uint32_t cus = (uint32_t)c->prop.multiProcessorCount;
                if (cus % w_xcd) w_xcd = 1;
                const int64_t cap = (int64_t)kBinsMaxLds / 4 - 96;
                w_slices = (uint32_t)((c->n_subjects + cap - 1) / cap);
                w_bins = ((uint32_t)c->n_subjects + w_slices - 1) / w_slices;  // slice = w_bins consecutive subject indices
                w_teams = (cus / w_xcd) / w_slices;
                if (!w_teams) weigh = false;
            }
            const int max_blocks = std::min(kStatBlocks, c->prop.multiProcessorCount * c->blocks_per_cu);
            const int blocks = grid_for(c->n_reads, c->threads, max_blocks);
            // dense bins: small id space, subject-indexed chunk, no size-normalised job
            int64_t bins = 0;
            int lds_slots = c->lds_slots;
            if (c->use_dense && c->subj_indexed && !by_subject && !hot_subjects && !weigh) {
                const int64_t b = std::max<int64_t>(c->n_nodes, (int64_t)c->max_subject_feature + 1);
                if (!sized && b * n_jobs <= 28672) {  // <= 112 KiB of bins + 32 KiB hash cache = 144 KiB LDS
                    bins = b;
                    lds_slots = std::min(lds_slots, 2048);
                    // two workgroups per CU fit if each stays below 80 KiB
                    if (c->blocks_per_cu >= 2 && b * n_jobs * 4 + 1024 * 16 <= 80 * 1024) lds_slots = 1024;
                }
            }
            size_t lds = (size_t)lds_slots * 16;
            // partitioned miss log: worth its fixed cost (one more merge
            // launch) only when many keys can miss the LDS cache
            uint32_t plog_cap = 0;
            // contributions that can reach the log: all of them, or — when the
            // single-candidate reads are counted per subject — those of the
            // multi-hit reads (each has >= 2 records, so at most twice the
            // excess of records over reads when no read is empty; an estimate,
            // the streams overflow into the count table)
            const int64_t contrib = by_subject ? 3 * std::max<int64_t>(c->n_records - c->n_reads, 0) + 1024
                                               : c->n_records + c->n_reads;
            if (!bins && !weigh && (c->use_plog == 2 || (c->use_plog == 1 && contrib >= (1 << 22)))) {
                // partitions: the merge counts a partition in one LDS table of
                // 8192 slots, so 256 partitions hold ~1.3 M distinct keys at a
                // comfortable load; fewer partitions keep a workgroup's open
                // log lines in L2 until they are full.  Distinct keys of a
                // launch <= sum over jobs of the ids the job can emit.
                int64_t distinct = 0;
                for (int j = 0; j < n_jobs; ++j) {
                    const int64_t ids = jobs[j].mode == WK_MODE_RANK   ? c->rank_tab_nodes[jobs[j].rank_slot]
                                        : jobs[j].mode == WK_MODE_FREE ? (int64_t)c->n_nodes
                                        : c->subj_indexed              ? (int64_t)c->n_subjects
                                        : c->n_genes > 0               ? (int64_t)c->n_genes
                                                                       : (int64_t)WK_MAX_FEATURE;
                    distinct += ids + 1;
                }
                const uint32_t log_parts = c->log_parts_opt ? (uint32_t)c->log_parts_opt
                                           : (!c->has_group && distinct <= 256 * 5120) ? 256u : kLogPartsMax;
                a.log_parts = log_parts;
                const int64_t streams = (int64_t)blocks * log_parts;
                // room for 3x the expected entries per stream if every contribution missed
                int64_t cap = 3 * (contrib * (int64_t)n_jobs / streams + 1) + 16;
                cap = std::min<int64_t>(cap, c->plog_max_bytes / 8 / streams);
                if (!sized && cap >= 16) {
                    plog_cap = (uint32_t)cap;
                    lds = (size_t)lds_slots * 16 + log_parts * 4;  // + the stream cursors
                    HIP_TRY(c, c->plog.reserve((size_t)streams * plog_cap * 8));
                    HIP_TRY(c, c->plog_cnt.reserve((size_t)streams * 4));
                    a.plog = c->plog.as<unsigned long long>();
                    a.plog_cnt = c->plog_cnt.as<uint32_t>();
                    a.plog_cap = plog_cap;
                }
            }
            if (bins) {
                lds += (size_t)bins * n_jobs * 4;
                HIP_TRY(c, c->dense_slab.reserve((size_t)blocks * bins * n_jobs * 4));
                a.dense_bins = (uint32_t)bins;
                a.dense_total = (uint32_t)(bins * n_jobs);
                a.dense_slab = c->dense_slab.as<uint32_t>();
            }
            if (weigh) {
                // ---- weighted subject histogram + per-subject merge; the reads it
                // does not cover go to the second pass below through a mask
                const uint32_t n_words = (uint32_t)((c->n_reads + 63) / 64);
                const uint32_t list_seg = (((n_words + 15u) / 16u + (uint32_t)blocks - 1u) / (uint32_t)blocks) * 1024u;
                const uint32_t n_teams = w_xcd * w_teams;
                HIP_TRY(c, c->left_list.reserve((size_t)blocks * list_seg * 4));
                HIP_TRY(c, c->w_slab.reserve((size_t)w_slices * n_teams * w_bins * 4));
                if ((size_t)c->n_subjects > c->w_hi_clean) {
                    HIP_TRY(c, c->w_hi.reserve((size_t)c->n_subjects * 4 + ((size_t)c->n_subjects * 4) / 2));
                    HIP_TRY(c, hipMemsetAsync(c->w_hi.p, 0, c->w_hi.cap, c->stream));
                    c->w_hi_clean = c->w_hi.cap / 4;
                }
                // which derivation of the read sizes: the one of the staging, or —
                // some subject lacks an ancestor at a rank in use — the one that
                // also leaves out the reads naming such a subject (once per staged
                // chunk and set of rank columns)
                int v = 0;
                if (c->rows_any_invalid) {
                    v = 1;
                    if (!c->rk_valid[1] || c->rk1_stage != c->stage_serial || c->rk1_rows != c->rows_serial) {
                        ktimer_end(c, kt);
                        kt = ktimer_begin(c, "read_sizes");
                        HIP_TRY(c, c->c_rk[1].reserve((size_t)c->n_records + 64));
                        HIP_TRY(c, c->rk_left[1].reserve((size_t)n_words * 8));
                        {
                            const int rc1 = derive_read_sizes(c, true, a.qoff, a.subj, c->n_reads, c->n_records,
                                                              c->c_rk[1].as<unsigned char>(),
                                                              c->rk_left[1].as<unsigned long long>(),
                                                              c->rk_totals.as<unsigned long long>() + 2);
                            if (rc1) return rc1;
                        }
                        ktimer_end(c, kt);
                        unsigned long long totals[2] = {0, 0};
                        HIP_TRY(c, hipMemcpyAsync(totals, c->rk_totals.as<unsigned char>() + 16, 16, hipMemcpyDeviceToHost, c->stream));
                        HIP_TRY(c, hipStreamSynchronize(c->stream));
                        c->rk_reads[1] = (int64_t)totals[0];
                        c->rk_records[1] = (int64_t)totals[1];
                        c->rk_valid[1] = true;
                        c->rk1_stage = c->stage_serial;
                        c->rk1_rows = c->rows_serial;
                        kt = ktimer_begin(c, "classify");
                    }
                }
                BinsArgs ba{};
                ba.subj = a.subj;
                ba.rk = c->c_rk[v].as<unsigned char>();
                ba.n_records = (uint32_t)c->n_records;
                ba.n_subjects = (uint32_t)c->n_subjects;
                ba.bins = w_bins;
                ba.n_slices = w_slices;
                ba.teams_per_xcd = w_teams;
                ba.n_xcd = w_xcd;
                ba.slab = c->w_slab.as<uint32_t>();
                ba.hi = c->w_hi.as<uint32_t>();
                ba.err = scalar_err(c);
                const dim3 wgrid((unsigned)c->prop.multiProcessorCount);
                const size_t wlds = ((size_t)w_bins + 96) * 4;
                kt = ktimer_begin(c, "classify");  // (again: the bracket starts at the launch, not at the host's decisions above)
                if (c->bins_ring == 6)
                    hipLaunchKernelGGL((weigh_bins_kernel<6>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
                else if (c->bins_ring == 8)
                    hipLaunchKernelGGL((weigh_bins_kernel<8>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
                else if (c->bins_ring == 3)
                    hipLaunchKernelGGL((weigh_bins_kernel<3>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
                else
                    hipLaunchKernelGGL((weigh_bins_kernel<4>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
                // (the reads and records it covers were counted with the sizes)
                c->stat_extra_reads += c->rk_reads[v];
                c->stat_extra_records += c->rk_records[v];
                ktimer_end(c, kt);
                kt = ktimer_begin(c, "weigh_merge");
                WeighMergeArgs wm{};
                wm.slab = ba.slab;
                wm.hi = ba.hi;
                wm.n_subjects = ba.n_subjects;
                wm.bins = w_bins;
                wm.n_teams = n_teams;
                wm.rows = a.rows;
                wm.row_w = a.row_w;
                wm.n_jobs = n_jobs;
                for (int j = 0; j < n_jobs; ++j) {
                    wm.mode[j] = a.jobs[j].mode;
                    wm.col[j] = a.jobs[j].col;
                    wm.job_id[j] = j;
                }
                wm.group = (uint32_t)a.group_base;
                wm.table = a.table;
                hipLaunchKernelGGL(weigh_merge_kernel, dim3((ba.n_subjects + kMergeSubjects - 1u) / kMergeSubjects), dim3(1024), (size_t)4096 * 16,
                                   c->stream, wm, 4096u);
                ktimer_end(c, kt);
                kt = ktimer_begin(c, "leftover");
                a.left_mask = c->rk_left[v].as<unsigned long long>();
                a.n_mask_words = n_words;
                a.list_seg = list_seg;
                a.read_list = c->left_list.as<uint32_t>();
                a.resume = 0;
                a.slab16 = 0;
            } else if (split) {
                // ---- first pass: single-candidate reads -----------------------------
                const uint32_t n_words = (uint32_t)((c->n_reads + 63) / 64);
                const uint32_t list_seg = (((n_words + 15u) / 16u + (uint32_t)blocks - 1u) / (uint32_t)blocks) * 1024u;
                HIP_TRY(c, c->left_mask.reserve((size_t)n_words * 8));
                HIP_TRY(c, c->left_list.reserve((size_t)blocks * list_seg * 4));
                unsigned long long* mask = c->left_mask.as<unsigned long long>();
                ClassifyArgs first = a;
                first.plog = nullptr;  // (kept when the first pass counts per read, below)
                first.plog_cnt = nullptr;
                first.plog_cap = 0;
                int blocks1 = blocks;
                if (by_subject) {
                    // its own grid and LDS layout: no hash cache to speak of, bins = subjects
                    blocks1 = grid_for((c->n_reads + 3) / 4, 1024,
                                       std::min(kStatBlocks, c->prop.multiProcessorCount * c->single_blocks_per_cu));
                    HIP_TRY(c, c->first_slab.reserve((size_t)blocks1 * ((size_t)c->n_subjects + 64) * 4));  // (16-bit layout pads units to 64 columns)
                    first.dense_bins = (uint32_t)c->n_subjects;
                    first.dense_total = (uint32_t)c->n_subjects;
                    first.dense_by_subject = 1;
                    first.dense_slab = c->first_slab.as<uint32_t>();
                    // reads per workgroup: its rounds x 4096
                    const int64_t rounds = ((c->n_reads + 4095) / 4096 + blocks1 - 1) / blocks1;
                    first.slab16 = rounds * 4096 <= 65535 ? 1 : 0;
                    if (c->use_count_kernel)
                        hipLaunchKernelGGL(count_subjects_kernel, dim3(blocks1), dim3(1024),
                                           64 * 16 + (size_t)c->n_subjects * 4, c->stream, first, 64u, mask);
                    else
                        hipLaunchKernelGGL((classify_single_kernel<true, true, 4>), dim3(blocks1), dim3(1024),
                                           64 * 16 + (size_t)c->n_subjects * 4, c->stream, first, 64u, mask);
                } else if (hot_subjects) {
                    // hash cache + log cursors like the second pass (shared streams),
                    // plus the hot subjects' bins behind them
                    HIP_TRY(c, c->first_slab.reserve((size_t)blocks * ((size_t)kHotBins + 64) * 4));
                    first.plog = a.plog;
                    first.plog_cnt = a.plog_cnt;
                    first.plog_cap = a.plog_cap;
                    first.dense_bins = kHotBins;
                    first.dense_total = kHotBins;
                    first.dense_by_subject = 1;
                    first.dense_slab = c->first_slab.as<uint32_t>();
                    const int64_t per_wg = ((c->n_reads + (int64_t)blocks * c->threads * 2 - 1) / ((int64_t)blocks * c->threads * 2)) * c->threads * 2;
                    first.slab16 = per_wg <= 65535 ? 1 : 0;
                    const int hot_slots = std::min(lds_slots, 2048);
                    const size_t lds1 = (size_t)hot_slots * 16 + (a.plog ? a.log_parts * 4 : 0) + (size_t)kHotBins * 4;
                    if (n_jobs == 1)
                        hipLaunchKernelGGL((classify_single_kernel<true, true, 2, false, true>), dim3(blocks), dim3(c->threads), lds1,
                                           c->stream, first, (uint32_t)hot_slots, mask);
                    else
                        hipLaunchKernelGGL((classify_single_kernel<true, false, 2, false, true>), dim3(blocks), dim3(c->threads), lds1,
                                           c->stream, first, (uint32_t)hot_slots, mask);
                } else {
                    // per-read evaluation with the same counting levels as the second
                    // pass; dense bins go to a slab of their own, log streams are shared
                    size_t lds1 = lds;
                    if (bins) {
                        HIP_TRY(c, c->first_slab.reserve((size_t)blocks * ((size_t)bins * n_jobs + 64) * 4));
                        first.dense_slab = c->first_slab.as<uint32_t>();
                        const int64_t per_wg = ((c->n_reads + (int64_t)blocks * c->threads - 1) / ((int64_t)blocks * c->threads)) * c->threads;
                        first.slab16 = per_wg <= 65535 ? 1 : 0;
                    } else {
                        first.plog = a.plog;
                        first.plog_cnt = a.plog_cnt;
                        first.plog_cap = a.plog_cap;
                    }
                    if (feature_chunk && n_jobs == 1)
                        hipLaunchKernelGGL((classify_single_kernel<false, true, kPerReadItems, true>), dim3(blocks), dim3(c->threads), lds1,
                                           c->stream, first, (uint32_t)lds_slots, mask);
                    else if (feature_chunk)
                        hipLaunchKernelGGL((classify_single_kernel<false, false, kPerReadItems, true>), dim3(blocks), dim3(c->threads), lds1,
                                           c->stream, first, (uint32_t)lds_slots, mask);
                    else if (n_jobs == 1)
                        hipLaunchKernelGGL((classify_single_kernel<false, true, kPerReadItems>), dim3(blocks), dim3(c->threads), lds1,
                                           c->stream, first, (uint32_t)lds_slots, mask);
                    else
                        hipLaunchKernelGGL((classify_single_kernel<false, false, kPerReadItems>), dim3(blocks), dim3(c->threads), lds1,
                                           c->stream, first, (uint32_t)lds_slots, mask);
                }
                ktimer_end(c, kt);
                kt = ktimer_begin(c, "leftover");
                // ---- second pass: merges the first pass's bins, lists and walks the rest
                a.left_mask = mask;
                a.n_mask_words = n_words;
                a.list_seg = list_seg;
                a.read_list = c->left_list.as<uint32_t>();
                if (by_subject || hot_subjects || bins) {
                    a.first_slab = c->first_slab.as<uint32_t>();
                    a.first_rows = (uint32_t)blocks1;
                    a.first_total = first.dense_total;
                    a.first_by_subject = (by_subject || hot_subjects) ? 1 : 0;
                    a.first_slab16 = first.slab16;
                }
                a.resume = (!by_subject && !bins && plog_cap) ? 1 : 0;
                a.slab16 = 0;
                if (bins) {  // the second pass counts in the hash cache only
                    a.dense_bins = 0;
                    a.dense_total = 0;
                    a.dense_slab = nullptr;
                    lds = (size_t)lds_slots * 16;
                    bins = 0;
                }
            }
            // one evaluator per kind of candidates (see classify_kernel's kPath)
            const int path = (a.rows != nullptr && a.row_w == 4) ? 0 : a.rows != nullptr ? 1 : 2;
            const dim3 grid(blocks), block(c->threads);
            if (ext) {
                const uint32_t n_words = (uint32_t)((c->n_reads + 63) / 64);
                const uint32_t list_seg = (((n_words + 15u) / 16u + (uint32_t)blocks - 1u) / (uint32_t)blocks) * 1024u;
                HIP_TRY(c, c->left_list.reserve((size_t)blocks * list_seg * 4));
                a.left_mask = c->left_mask.as<unsigned long long>();
                a.n_mask_words = n_words;
                a.list_seg = list_seg;
                a.read_list = c->left_list.as<uint32_t>();
                a.resume = 0;
                a.slab16 = 0;
            }
            const bool listed = split || weigh || ext;
            if (listed && path == 0)
                hipLaunchKernelGGL((classify_kernel<true, true, 0>), grid, block, lds, c->stream, a, (uint32_t)lds_slots);
            else if (listed && path == 1)
                hipLaunchKernelGGL((classify_kernel<true, true, 1>), grid, block, lds, c->stream, a, (uint32_t)lds_slots);
            else if (listed)
                hipLaunchKernelGGL((classify_kernel<true, true, 2>), grid, block, lds, c->stream, a, (uint32_t)lds_slots);
            else if (path == 0)
                hipLaunchKernelGGL((classify_kernel<true, false, 0>), grid, block, lds, c->stream, a, (uint32_t)lds_slots);
            else if (path == 1)
                hipLaunchKernelGGL((classify_kernel<true, false, 1>), grid, block, lds, c->stream, a, (uint32_t)lds_slots);
            else
                hipLaunchKernelGGL((classify_kernel<true, false, 2>), grid, block, lds, c->stream, a, (uint32_t)lds_slots);
            if (plog_cap) {
                ktimer_end(c, kt);
                kt = ktimer_begin(c, "partition_merge");
                hipLaunchKernelGGL(partition_merge_kernel, dim3(a.log_parts), dim3(1024), (size_t)8192 * 16, c->stream,
                                   c->plog.as<unsigned long long>(), c->plog_cnt.as<uint32_t>(), (uint32_t)blocks,
                                   plog_cap, 8192u, a.table);
            }
            if (bins) {
                ktimer_end(c, kt);
                kt = ktimer_begin(c, "dense_merge");
                const uint32_t nb = (uint32_t)(bins * n_jobs);
                hipLaunchKernelGGL(dense_merge_kernel, dim3((nb + 63) / 64), dim3(1024), 0, c->stream,
                                   c->dense_slab.as<uint32_t>(), (uint32_t)blocks, (uint32_t)n_jobs, (uint32_t)bins, (uint32_t)a.group_base, a.table);
            }
        } else {
            const int blocks = grid_for(c->n_reads, 256, c->prop.multiProcessorCount * 8);
            hipLaunchKernelGGL(classify_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, a, 0u);
        }
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
    }
    if (out_assign) {
        HIP_TRY(c, hipMemcpyAsync(out_assign, c->assign_out.p, (size_t)n_jobs * (size_t)c->n_reads * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return WK_OK;
}

int wk_classify_chunk(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, const int32_t* subj, const int32_t* qoff,
                      int64_t n_reads, const int32_t* group, int subj_flags, int32_t* out_assign) {
    int rc = wk_chunk_stage(c, subj, qoff, n_reads, group, subj_flags);
    if (rc) return rc;
    return wk_classify_staged(c, jobs, n_jobs, out_assign);
}

// ---- packed records accumulated over the chunks of a sample ---------------------

int wk_host_alloc(wk_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return WK_E_ARG;
    DeviceGuard guard(c->device);
    void* p = nullptr;
    HIP_TRY(c, hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault));
    {
        std::lock_guard<std::mutex> lock(c->host_mu);
        c->host_blocks.push_back(p);
    }
    *out = p;
    return WK_OK;
}

int wk_host_free(wk_ctx* c, void* p) {
    if (!c || !p) return WK_E_ARG;
    {
        std::lock_guard<std::mutex> lock(c->host_mu);
        auto it = std::find(c->host_blocks.begin(), c->host_blocks.end(), p);
        if (it == c->host_blocks.end()) return fail(c, WK_E_ARG, "not a block of wk_host_alloc");
        c->host_blocks.erase(it);
    }
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipHostFree(p));
    return WK_OK;
}

// Can the weighted histogram alone classify records under these jobs?  Plain
// assigners only (see wk_weigh.hpp) and — checked against the current subject
// table — every subject with an ancestor at every rank in use.
// Does the job look at whole reads (the per-read stream of wk_free.hpp)?  `--rank free`, or a rank under --uniq, --above
// or --major above one half; never a size-normalised job.
static bool job_whole_reads(const wk_job& jb) {
    if (jb.flags & WK_F_SIZED) return false;
    if (jb.mode == WK_MODE_FREE) return true;
    return jb.mode == WK_MODE_RANK && (jb.major > 0.5 || (jb.major <= 0.0 && (jb.flags & (WK_F_UNIQ | WK_F_ABOVE))));
}

// `mixed` (wk_words_begin_mixed): a set of whole-read jobs next to plain ones is taken too, as mode 4.  `a` then holds
// the plain jobs alone, in the order of the set (a.n_jobs of them), and `plain_ids` (may be null) their indices in it.
static int words_jobs_ok(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, ClassifyArgs& a, bool* ok, int* mode = nullptr,
                         bool mixed = false, int32_t* plain_ids = nullptr) {
    *ok = false;
    if (mode) *mode = 0;
    if (!c->use_weigh || c->n_subjects <= 0 || c->n_subjects > (int32_t)kWordSubjMask + 1) return WK_OK;
    // Jobs that look at whole reads — `--rank free` (classify.assign_free), a rank under --uniq, --above or --major above
    // one half (classify.assign_rank) — go to the per-read stream over node ids (wk_free.hpp): one such job with the
    // records rewritten as they are appended, several with the records rewritten per job when the sample is classified.
    int n_stream = 0;
    for (int j = 0; j < n_jobs; ++j) n_stream += job_whole_reads(jobs[j]) ? 1 : 0;
    const bool mix = mixed && n_stream > 0 && n_stream < n_jobs;
    bool stream_refuses = false;  // (a mixed set: its rows are built all the same, for the flush of what has been accumulated)
    {
        if ((n_stream == n_jobs && n_jobs >= 1) || mix) {
            if (c->n_nodes <= 0 || (uint32_t)c->n_nodes >= kFreeMissing) return WK_OK;
            for (int j = 0; j < n_jobs; ++j) {
                const wk_job& jb = jobs[j];
                if (!job_whole_reads(jb)) continue;  // (a mixed set's plain jobs: below)
                if (jb.mode == WK_MODE_FREE) {
                    if (jb.flags & WK_F_SUBOK)  // a subject that is no node is its own result under --subok: not a feature the stream can carry
                        for (int32_t f : c->subj_feat_host)
                            if (f >= c->n_nodes) {
                                if (!mix) return WK_OK;
                                stream_refuses = true;
                                break;
                            }
                } else if (jb.rank_slot < 0 || jb.rank_slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) ||
                           !c->rank_tab_valid[jb.rank_slot]) {
                    return fail(c, WK_E_STATE, "job %d: rank slot %d has not been built", j, jb.rank_slot);
                }
            }
            if (!mix) {
                if (mode) *mode = n_jobs > 1 ? 3 : jobs[0].mode == WK_MODE_FREE ? 1 : 2;
                *ok = true;
                return WK_OK;
            }
        }
    }
    if (mix) {
        // ---- the plain jobs of a mixed set: the checks and the subject rows of a plain set, over them alone
        wk_job plain[WK_MAX_JOBS];
        int32_t n_plain = 0;
        a = ClassifyArgs{};
        for (int j = 0; j < n_jobs; ++j) {
            const wk_job& jb = jobs[j];
            if (job_whole_reads(jb)) continue;
            if (jb.flags & (WK_F_SIZED | WK_F_UNIQ)) return WK_OK;
            if (jb.mode == WK_MODE_RANK) {
                if ((jb.flags & WK_F_ABOVE) || jb.major > 0.0) return WK_OK;
                if (jb.rank_slot < 0 || jb.rank_slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) || !c->rank_tab_valid[jb.rank_slot])
                    return fail(c, WK_E_STATE, "job %d: rank slot %d has not been built", j, jb.rank_slot);
            } else if (jb.mode != WK_MODE_NONE) {
                return WK_OK;
            }
            JobDev d{};
            d.mode = jb.mode;
            d.flags = jb.flags;
            d.major = jb.major;
            a.jobs[n_plain] = d;
            if (plain_ids) plain_ids[n_plain] = j;
            plain[n_plain++] = jb;
        }
        a.n_jobs = n_plain;
        const int rc = build_subject_rows(c, plain, n_plain, a);
        if (rc) return rc;
        *ok = !c->rows_any_invalid && !stream_refuses;
        if (mode) *mode = 4;
        return WK_OK;
    }
    a = ClassifyArgs{};
    a.n_jobs = n_jobs;
    // Size-normalised plain jobs (classify.counter_size, classify.py:174-213) are taken when the whole set is such jobs:
    // their flush is the histogram over (subject, read size) of wk_sized.hpp.  Next to unsized jobs they are refused.
    int n_sized = 0;
    for (int j = 0; j < n_jobs; ++j) n_sized += (jobs[j].flags & WK_F_SIZED) ? 1 : 0;
    if (n_sized && n_sized != n_jobs) return WK_OK;
    for (int j = 0; j < n_jobs; ++j) {
        const wk_job& jb = jobs[j];
        if (jb.flags & WK_F_UNIQ) return WK_OK;
        if (jb.mode == WK_MODE_RANK) {
            if ((jb.flags & WK_F_ABOVE) || jb.major > 0.0) return WK_OK;
            if (c->n_nodes <= 0) return fail(c, WK_E_STATE, "job %d needs a hierarchy (wk_set_tree)", j);
            if (jb.rank_slot < 0 || jb.rank_slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) || !c->rank_tab_valid[jb.rank_slot])
                return fail(c, WK_E_STATE, "job %d: rank slot %d has not been built", j, jb.rank_slot);
        } else if (jb.mode != WK_MODE_NONE) {
            return WK_OK;
        }
        JobDev d{};
        d.mode = jb.mode;
        d.flags = jb.flags;
        d.major = jb.major;
        a.jobs[j] = d;
    }
    const int rc = build_subject_rows(c, jobs, n_jobs, a);
    if (rc) return rc;
    *ok = !c->rows_any_invalid;
    return WK_OK;
}

static bool same_jobs(const std::vector<wk_job>& have, const wk_job* jobs, int32_t n) {
    if ((int32_t)have.size() != n) return false;
    for (int32_t j = 0; j < n; ++j)
        if (have[j].mode != jobs[j].mode || have[j].rank_slot != jobs[j].rank_slot || have[j].flags != jobs[j].flags ||
            have[j].major != jobs[j].major)
            return false;
    return true;
}

// Room for `need` rows in the pile of distinct rows (sz_rows / sz_counts): new buffers (twice the need) take over the
// rows held.
static int sized_pile_reserve(wk_ctx* c, size_t need) {
    if (need * 16 <= c->sz_rows.cap && need * 8 <= c->sz_counts.cap) return WK_OK;
    DevBuf rows, counts;
    HIP_TRY(c, rows.reserve(need * 2 * 16));
    hipError_t e = counts.reserve(need * 2 * 8);
    if (e != hipSuccess) {
        rows.release();
        HIP_TRY(c, e);
    }
    if (c->sz_n > 0) {
        (void)hipMemcpyAsync(rows.p, c->sz_rows.p, (size_t)c->sz_n * 16, hipMemcpyDeviceToDevice, c->stream);
        (void)hipMemcpyAsync(counts.p, c->sz_counts.p, (size_t)c->sz_n * 8, hipMemcpyDeviceToDevice, c->stream);
    }
    e = hipStreamSynchronize(c->stream);
    c->sz_rows.release();
    c->sz_counts.release();
    c->sz_rows = rows;
    c->sz_counts = counts;
    HIP_TRY(c, e);
    return WK_OK;
}

// The flush of a job set of size-normalised plain jobs (wk_sized.hpp): the table C[subject][read size] of the sample's
// record streams, then one row per non-zero bin and job behind the rows of earlier flushes (wk_sized_fetch takes them).
static int words_flush_sized(wk_ctx* c, const ClassifyArgs& a) {
    const int32_t n_jobs = (int32_t)c->w_jobs.size();
    const uint32_t cus = (uint32_t)c->prop.multiProcessorCount;
    const int S = c->w_sliced ? c->w_streams : 1;
    // sub-slices of every stream, and teams in proportion to its records: about one workgroup per CU in all
    uint32_t n_q[kMaxStreams] = {}, teams[kMaxStreams] = {}, row_first[kMaxStreams] = {};
    unsigned long long total = 0;
    for (int k = 0; k < S; ++k) {
        if (c->w_count[k] >= (1ull << 30)) return fail(c, WK_E_RANGE, "more than 2^30 records in one stream");
        if (!c->w_count[k]) continue;
        const int64_t lo = c->w_sliced ? (int64_t)k * kSliceBins : 0;
        const int64_t held = std::max<int64_t>(0, c->w_sliced ? std::min<int64_t>(c->n_subjects - lo, kSliceBins) : c->n_subjects);
        n_q[k] = (uint32_t)std::max<int64_t>(1, (held + kSizedSub - 1) / kSizedSub);
        total += c->w_count[k];
    }
    uint32_t n_rows = 0;
    for (int k = 0; k < S; ++k) {
        if (!n_q[k]) continue;
        const unsigned long long share = (unsigned long long)cus * c->w_count[k] / std::max<unsigned long long>(total, 1);  // workgroups this stream may have
        const unsigned long long tiles = (c->w_count[k] + kSizedTile - 1) / kSizedTile;
        uint32_t t = (uint32_t)std::max<unsigned long long>(1, std::min(share / n_q[k], tiles));
        if (t >= 8u) t &= ~7u;  // (whole octets: a team on one XCD)
        teams[k] = t;
        row_first[k] = n_rows;
        n_rows += n_q[k] * t;
    }
    HIP_TRY(c, c->w_slab.reserve((size_t)std::max(n_rows, 1u) * kSliceBins * 4));
    HIP_TRY(c, c->sz_scal.reserve(16));
    HIP_TRY(c, hipMemsetAsync(c->sz_scal.p, 0, 16, c->stream));
    KernelTimer* kt = ktimer_begin(c, "sized_bins");
    for (int k = 0; k < S; ++k) {
        if (!n_q[k]) continue;
        SizedBinsArgs ba{};
        ba.words = c->w_stream[k].as<uint32_t>();
        ba.n_records = (uint32_t)c->w_count[k];
        ba.n_subjects = (uint32_t)c->n_subjects;
        ba.q_first = c->w_sliced ? (uint32_t)k * kSizedSizes : 0u;
        ba.n_q = n_q[k];
        ba.n_teams = teams[k];
        ba.slab = c->w_slab.as<uint32_t>() + (size_t)row_first[k] * kSliceBins;
        ba.err = scalar_err(c);
        hipLaunchKernelGGL((sized_bins_kernel<4>), dim3(n_q[k] * teams[k]), dim3(kSizedThreads), (size_t)kSliceBins * 4, c->stream, ba);
    }
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    SizedRowsArgs ra{};
    ra.slab = c->w_slab.as<uint32_t>();
    // (a subject table that grew past the streams' slices since they were opened holds no records behind them)
    ra.n_subjects = (uint32_t)(c->w_sliced ? std::min<int64_t>(c->n_subjects, (int64_t)S * kSliceBins) : c->n_subjects);
    ra.sliced = c->w_sliced ? 1u : 0u;
    for (int k = 0; k < S; ++k) {
        ra.teams[k] = teams[k];
        ra.row_first[k] = row_first[k];
    }
    ra.rows = a.rows;
    ra.row_w = a.row_w;
    ra.n_jobs = n_jobs;
    for (int j = 0; j < n_jobs; ++j) {
        ra.mode[j] = a.jobs[j].mode;
        ra.col[j] = a.jobs[j].col;
    }
    ra.group = c->w_group;
    ra.n_bins = c->sz_scal.as<unsigned long long>();
    ra.cursor = c->sz_scal.as<unsigned long long>() + 1;
    ra.err = scalar_err(c);
    const dim3 rgrid((kSliceBins + kSizedRowsThreads - 1) / kSizedRowsThreads, std::max(1u, (ra.n_subjects + kSizedSub - 1) / kSizedSub));
    kt = ktimer_begin(c, "sized_rows");
    hipLaunchKernelGGL((sized_rows_kernel<false>), rgrid, dim3(kSizedRowsThreads), 0, c->stream, ra);
    HIP_TRY(c, hipGetLastError());
    unsigned long long n_bins = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_bins, c->sz_scal.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t more = (int64_t)n_bins * n_jobs;
    if (more > 0) {
        const size_t need = (size_t)(c->sz_n + more);
        const int grown = sized_pile_reserve(c, need);
        if (grown) return grown;
        ra.out_rows = c->sz_rows.as<int4>();
        ra.out_counts = c->sz_counts.as<long long>();
        ra.base = (unsigned long long)c->sz_n;
        ra.cap = (unsigned long long)need;
        hipLaunchKernelGGL((sized_rows_kernel<true>), rgrid, dim3(kSizedRowsThreads), 0, c->stream, ra);
        HIP_TRY(c, hipGetLastError());
        c->sz_n += more;
        c->sz_flushes += 1;
    }
    ktimer_end(c, kt);
    c->stat_extra_reads += c->w_reads;
    c->stat_extra_records += c->w_records;
    if (c->words_keep) return WK_OK;
    return words_reset(c);
}

int wk_sized_pending(wk_ctx* c, int64_t* n_rows, int64_t* n_flushes) {
    if (!c) return WK_E_ARG;
    if (n_rows) *n_rows = c->sz_n;
    if (n_flushes) *n_flushes = c->sz_flushes;
    return WK_OK;
}

int wk_sized_fetch(wk_ctx* c, int32_t* rows, int64_t* counts, int64_t cap, int64_t* n) {
    if (!c || !n) return WK_E_ARG;
    DeviceGuard guard(c->device);
    int rc = c->words_keep ? WK_OK : wk_words_flush(c);  // records still accumulated (wk_words_append) become rows now
    if (rc) return rc;
    if ((rc = check_device_errors(c))) return rc;
    *n = c->sz_n;
    if (c->sz_n > cap || (c->sz_n && (!rows || !counts)))
        return fail(c, WK_E_CAPACITY, "output capacity %lld < %lld rows", (long long)cap, (long long)c->sz_n);
    if (c->sz_n == 0) return WK_OK;
    HIP_TRY(c, hipMemcpyAsync(rows, c->sz_rows.p, (size_t)c->sz_n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts, c->sz_counts.p, (size_t)c->sz_n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sz_n = 0;
    return WK_OK;
}

// The contribution log of the chunk just classified as distinct rows with counts, behind the rows of the pile
// (wk_logred.hpp); the log is emptied.
int wk_log_reduce(wk_ctx* c, int64_t* n_rows_in, int64_t* n_distinct) {
    if (!c || !n_rows_in || !n_distinct) return WK_E_ARG;
    DeviceGuard guard(c->device);
    *n_rows_in = *n_distinct = 0;
    int rc = check_device_errors(c);
    if (rc) return rc;
    unsigned long long used = 0;
    HIP_TRY(c, hipMemcpyAsync(&used, scalar_u64(c, 5), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_rows_in = (int64_t)used;
    if (used == 0) return WK_OK;
    if ((int64_t)used > c->log_cap) {
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 5), 0, 8, c->stream));
        return fail(c, WK_E_CAPACITY, "contribution log overflowed: %llu entries needed, %lld reserved", used, (long long)c->log_cap);
    }
    // (the cursor stays: a call that fails below leaves the log to wk_log_fetch)
    if (used >= (1ull << 31)) return fail(c, WK_E_RANGE, "a log of %llu rows cannot be reduced on the device (row indices are 32 bits); use wk_log_fetch", used);
    KtScope kt_scope(c);
    uint64_t slots = 1024;
    while (slots < 2 * used) slots <<= 1;
    HIP_TRY(c, c->lr_table.reserve((size_t)slots * 8));
    HIP_TRY(c, c->sz_scal.reserve(16));
    uint32_t* const tidx = c->lr_table.as<uint32_t>();
    uint32_t* const tcnt = tidx + slots;
    HIP_TRY(c, hipMemsetAsync(tidx, 0xFF, (size_t)slots * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(tcnt, 0, (size_t)slots * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->sz_scal.p, 0, 16, c->stream));
    LogReduceArgs ra{};
    ra.log = c->log.as<int4>();
    ra.n_rows = (uint32_t)used;
    ra.tidx = tidx;
    ra.tcnt = tcnt;
    ra.mask = (uint32_t)(slots - 1);
    ra.n_distinct = c->sz_scal.as<unsigned long long>();
    ra.err = scalar_err(c);
    const uint64_t wgs = std::min<uint64_t>((used + kLogRedThreads - 1) / kLogRedThreads, (uint64_t)c->prop.multiProcessorCount * kLogRedWgPerCu);
    KernelTimer* kt = ktimer_begin(c, "log_reduce");
    hipLaunchKernelGGL(log_reduce_kernel, dim3((unsigned)wgs), dim3(kLogRedThreads), kLogRedFrontBytes, c->stream, ra);
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    unsigned long long distinct = 0;
    HIP_TRY(c, hipMemcpyAsync(&distinct, c->sz_scal.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (distinct == 0 || distinct > used) return fail(c, WK_E_HIP, "log reduction counted %llu distinct rows of %llu", distinct, used);
    const size_t need = (size_t)c->sz_n + (size_t)distinct;
    if ((rc = sized_pile_reserve(c, need))) return rc;
    LogEmitArgs ea{};
    ea.log = ra.log;
    ea.n_rows = ra.n_rows;
    ea.tidx = tidx;
    ea.tcnt = tcnt;
    ea.slots = slots;
    ea.out_rows = c->sz_rows.as<int4>();
    ea.out_counts = c->sz_counts.as<long long>();
    ea.cursor = c->sz_scal.as<unsigned long long>() + 1;
    ea.base = (unsigned long long)c->sz_n;
    ea.cap = (unsigned long long)need;
    ea.err = scalar_err(c);
    kt = ktimer_begin(c, "log_emit");
    hipLaunchKernelGGL(log_emit_kernel, dim3((unsigned)((slots + kLogRedEmitThreads - 1) / kLogRedEmitThreads)), dim3(kLogRedEmitThreads), 0, c->stream, ea);
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    c->sz_n += (int64_t)distinct;
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 5), 0, 8, c->stream));
    *n_distinct = (int64_t)distinct;
    return WK_OK;
}

// teams per XCD of the team layout over the unsliced stream; 0: the table has more slices than a team has workgroups
static uint32_t words_team_size(const wk_ctx* c) {
    const uint32_t cus = (uint32_t)c->prop.multiProcessorCount;
    const uint32_t w_xcd = cus % 8u ? 1u : 8u;
    return (cus / w_xcd) / (uint32_t)streams_needed(c);
}

int wk_words_flush(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    if (c->lag_count) return fail(c, WK_E_STATE, "blocks whose verdict has not been read (wk_dtok_scan_emit_end)");
    if (!c->w_open || c->w_records == 0) return words_reset(c);
    if (!c->slots) return fail(c, WK_E_STATE, "count table not reserved (wk_counts_reserve)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    if (c->w_mode != 0) {
        // ---- free-rank jobs and rank jobs that look at whole reads: per job, the stream over node ids, then its dense
        // counters into the count table.  One job: the records hold its node ids since they were appended; several:
        // they hold subject indices, which the stream reads through the job's table (free_stream_kernel<., true>).  A
        // mixed set (mode 4): its whole-read jobs as the several of mode 3, each under its index in the set; the plain
        // jobs are counted from the same records by the weighted histogram below.
        const int blocks = std::min(kStatBlocks, c->prop.multiProcessorCount * c->free_per_cu);
        const CountTable table{c->tkeys.as<unsigned long long>(), c->tvals.as<unsigned long long>(), c->slots - 1, scalar_err(c)};
        if (c->w_mode != 3 && c->w_mode != 4) {  // (subjects registered since the last chunk was appended)
            const int rcr = refresh_word_ranks(c, c->w_records);
            if (rcr) return rcr;
        }
        bool stats_counted = false;
        for (size_t j = 0; j < c->w_jobs.size(); ++j) {
            const wk_job& jb = c->w_jobs[j];
            if (c->w_mode == 4 && !job_whole_reads(jb)) continue;
            const int kind = jb.mode == WK_MODE_FREE ? 1 : 2;
            wk_ctx::StreamTables& T = c->st[j];
            {
                const int rcf = ensure_stream_tables(c, T, kind, kind == 2 ? jb.rank_slot : -1);
                if (rcf) return rcf;
            }
            FreeArgs fa{};
            fa.words = c->c_words.as<uint32_t>();
            const bool translate = c->w_mode >= 3;  // (several jobs: the records hold subject indices, read through this job's table)
            fa.rank_of_subject = translate ? T.subj_rank.as<int32_t>() : nullptr;
            fa.n_subjects = (uint32_t)c->n_subjects;
            fa.err = scalar_err(c);
            fa.sparse = T.dsparse.as<int32_t>();
            fa.parent_d = T.dparent.as<int32_t>();
            fa.self_d = T.dself.as<int32_t>();
            fa.sparse_m = T.dm;
            fa.n_records = (uint32_t)c->w_records;
            fa.job = (uint32_t)j;
            fa.group = (uint32_t)c->w_group;
            fa.subok = (jb.flags & WK_F_SUBOK) ? 1u : 0u;
            fa.unassigned = (jb.flags & WK_F_UNASSIGNED) ? 1u : 0u;
            fa.by_rank = kind == 2 ? 1u : 0u;
            fa.above = (jb.flags & WK_F_ABOVE) ? 1u : 0u;
            fa.major = kind == 2 ? jb.major : 0.0;
            fa.count_stats = stats_counted ? 0u : 1u;  // (reads and records are counted once, by the first such job)
            stats_counted = true;
            // the dense counters of the results (zero between launches: free_counts_kernel clears what it moves)
            const size_t dense_bytes = ((size_t)T.results + 1) * 4;
            if (c->f_dense.cap < dense_bytes || c->f_dense_tree != c->tree_serial) {  // (otherwise zero)
                HIP_TRY(c, c->f_dense.reserve(dense_bytes));
                HIP_TRY(c, hipMemsetAsync(c->f_dense.p, 0, c->f_dense.cap, c->stream));
                c->f_dense_tree = c->tree_serial;
            }
            fa.dense = c->f_dense.as<uint32_t>();
            fa.n_results = T.results;
            fa.stat_block = c->stat_block.as<unsigned long long>();
            const uint32_t slots = (uint32_t)c->free_slots;
            const size_t lds = (size_t)slots * 8 + (size_t)(c->free_threads / 64) * free_wave_lds();
            // a wave's list of uncached results: room for every read it can meet (240 per block of records)
            const uint32_t n_waves = (uint32_t)blocks * (uint32_t)(c->free_threads / 64);
            const uint32_t n_blocks = (fa.n_records + kFreeAdvance - 1) / kFreeAdvance;
            fa.log_cap = ((n_blocks + n_waves - 1) / n_waves * kFreeAdvance + 63u) / 64u * 64u;
            const uint32_t n_slices = (T.results + 1 + kLogBins - 1) / kLogBins;
            HIP_TRY(c, c->f_log.reserve((size_t)n_waves * fa.log_cap * 4));
            HIP_TRY(c, c->f_log_cnt.reserve((size_t)n_waves * 4));
            // (shares x slices = workgroups of free_log_kernel, one per CU: as many as run at once)
            const uint32_t n_parts = std::max(8u, std::min(kListSharesMax, ((uint32_t)c->prop.multiProcessorCount / n_slices) & ~7u));
            HIP_TRY(c, c->f_partial.reserve((size_t)n_parts * n_slices * kLogBins * 4));
            HIP_TRY(c, c->f_part_used.reserve((size_t)n_parts * n_slices * 4));
            fa.log = c->f_log.as<uint32_t>();
            fa.log_cnt = c->f_log_cnt.as<uint32_t>();
            KernelTimer* kt = ktimer_begin(c, "classify");
            if (fa.major > 0.0 && translate)
                hipLaunchKernelGGL((free_stream_kernel<true, true>), dim3(blocks), dim3(c->free_threads), lds, c->stream, fa, slots);
            else if (fa.major > 0.0)
                hipLaunchKernelGGL((free_stream_kernel<true, false>), dim3(blocks), dim3(c->free_threads), lds, c->stream, fa, slots);
            else if (translate)
                hipLaunchKernelGGL((free_stream_kernel<false, true>), dim3(blocks), dim3(c->free_threads), lds, c->stream, fa, slots);
            else
                hipLaunchKernelGGL((free_stream_kernel<false, false>), dim3(blocks), dim3(c->free_threads), lds, c->stream, fa, slots);
            ktimer_end(c, kt);
            FreeLogArgs la{};
            la.log = fa.log;
            la.log_cnt = fa.log_cnt;
            la.log_cap = fa.log_cap;
            la.n_waves = n_waves;
            la.n_slices = n_slices;
            la.n_parts = n_parts;
            la.partial = c->f_partial.as<uint32_t>();
            la.part_used = c->f_part_used.as<uint32_t>();
            kt = ktimer_begin(c, "free_log");
            hipLaunchKernelGGL(free_log_kernel, dim3(n_parts * n_slices), dim3(kLogThreads), (size_t)kLogBins * 4, c->stream, la);
            ktimer_end(c, kt);
            kt = ktimer_begin(c, "free_counts");
            hipLaunchKernelGGL(free_counts_kernel, dim3((T.results + 256) / 256), dim3(256), 0, c->stream, fa.dense, fa.n_results,
                               T.rnode.as<int32_t>(), fa.job, fa.group, la.partial, la.part_used, n_slices, n_parts, table);
            ktimer_end(c, kt);
            HIP_TRY(c, hipGetLastError());
        }
        if (c->w_mode != 4) {
            if (c->words_keep) return WK_OK;
            return words_reset(c);
        }
    }
    const bool mixed = c->w_mode == 4;
    ClassifyArgs a{};
    bool ok = false;
    int32_t job_id[WK_MAX_JOBS];
    for (int j = 0; j < WK_MAX_JOBS; ++j) job_id[j] = j;
    int rc = words_jobs_ok(c, c->w_jobs.data(), (int32_t)c->w_jobs.size(), a, &ok, nullptr, mixed, job_id);
    if (rc) return rc;
    if (mixed && !a.rows) return fail(c, WK_E_STATE, "the plain jobs of the mixed set have no subject rows");
    // (`ok` may be false by now: a subject without an ancestor at a rank in use
    // joined the table after these records.  wk_words_begin stops accepting
    // records the moment that happens, so every subject the accumulated records
    // name has a valid row — rows of old subjects do not change when the table
    // grows — and the new ones carry no weight.)
    (void)ok;
    const int32_t n_jobs = mixed ? a.n_jobs : (int32_t)c->w_jobs.size();  // (a mixed set: its plain jobs, `job_id` their places in it)
    const uint32_t cus = (uint32_t)c->prop.multiProcessorCount;
    // the one unsliced stream of the branches below: the first stream of the histogram's own accumulation, or a mixed
    // set's records in read order
    const uint32_t* const one_words = mixed ? c->c_words.as<uint32_t>() : c->w_stream[0].as<uint32_t>();
    // how many records every stream holds (known once per accumulation state)
    if (!mixed && !c->w_counts_known) {
        HIP_TRY(c, hipMemcpyAsync(c->w_count, c->w_cursor.p, kMaxStreams * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->w_counts_known = true;
    }
    if (c->w_jobs[0].flags & WK_F_SIZED) return words_flush_sized(c, a);
    if ((size_t)c->n_subjects > c->w_hi_clean) {
        HIP_TRY(c, c->w_hi.reserve((size_t)c->n_subjects * 4 + ((size_t)c->n_subjects * 4) / 2));
        HIP_TRY(c, hipMemsetAsync(c->w_hi.p, 0, c->w_hi.cap, c->stream));
        c->w_hi_clean = c->w_hi.cap / 4;
    }
    const unsigned long long one_count = mixed ? (unsigned long long)c->w_records : c->w_count[0];
    WeighMergeArgs wm{};
    KernelTimer* kt = nullptr;
    if (c->w_sliced && !mixed) {
        // ---- a stream per slice of the subject table, each read once; workgroups in proportion to the streams' lengths
        StreamBinsArgs sa{};
        const int S = c->w_streams;
        unsigned long long total = 0;
        for (int k = 0; k < S; ++k) total += c->w_count[k];
        uint32_t wg[kMaxStreams] = {}, used = 0;
        for (int k = 0; k < S; ++k)
            if (c->w_count[k]) {
                wg[k] = (uint32_t)std::max<unsigned long long>(1, c->w_count[k] * cus / total);
                used += wg[k];
            }
        while (used > cus) {  // (the minimum of one workgroup per stream pushed the sum over)
            int big = 0;
            for (int k = 1; k < S; ++k)
                if (wg[k] > wg[big]) big = k;
            --wg[big];
            --used;
        }
        while (used < cus && total) {  // what the rounding left: to the stream with the most records per workgroup
            int best = -1;
            for (int k = 0; k < S; ++k)
                if (wg[k] && (best < 0 || c->w_count[k] * wg[best] > c->w_count[best] * wg[k])) best = k;
            ++wg[best];
            ++used;
        }
        sa.n_streams = (uint32_t)S;
        sa.n_subjects = (uint32_t)c->n_subjects;
        uint32_t first = 0;
        for (int k = 0; k < S; ++k) {
            if (c->w_count[k] >= (1ull << 30)) return fail(c, WK_E_RANGE, "more than 2^30 records in one stream");
            sa.words[k] = c->w_stream[k].as<uint32_t>();
            sa.count[k] = (uint32_t)c->w_count[k];
            sa.wg_first[k] = first;
            first += wg[k];
        }
        for (int k = S; k <= kMaxStreams; ++k) sa.wg_first[k] = first;
        const uint32_t n_wg = first;
        HIP_TRY(c, c->w_slab.reserve((size_t)std::max(n_wg, 1u) * kSliceBins * 4));
        sa.slab = c->w_slab.as<uint32_t>();
        sa.hi = c->w_hi.as<uint32_t>();
        sa.err = scalar_err(c);
        kt = ktimer_begin(c, "classify");
        if (n_wg) {
            if (c->bins_ring == 6)
                hipLaunchKernelGGL((weigh_streams_kernel<6>), dim3(n_wg), dim3(kWeighThreads), kBinsMaxLds, c->stream, sa);
            else if (c->bins_ring == 8)
                hipLaunchKernelGGL((weigh_streams_kernel<8>), dim3(n_wg), dim3(kWeighThreads), kBinsMaxLds, c->stream, sa);
            else
                hipLaunchKernelGGL((weigh_streams_kernel<4>), dim3(n_wg), dim3(kWeighThreads), kBinsMaxLds, c->stream, sa);
        }
        ktimer_end(c, kt);
        wm.slab = sa.slab;
        wm.hi = sa.hi;
        wm.streams = (uint32_t)S;
        for (int k = 0; k <= kMaxStreams; ++k) wm.wg_first[k] = sa.wg_first[k];
        wm.bins = kSliceBins;
        wm.n_teams = 0;
    } else if (c->weigh_wide || words_team_size(c) == 0) {
        // ---- more slices than a team has workgroups (wk_weigh_wide.hpp): the one stream partitioned by slice, then every
        // bucket read once
        if (one_count >= (1ull << 30)) return fail(c, WK_E_RANGE, "more than 2^30 records in one stream");
        const uint32_t n = (uint32_t)one_count;
        const uint32_t n_buckets = (uint32_t)streams_needed(c);  // (at most kWideMaxBuckets: words_jobs_ok)
        const uint32_t n_wg = std::min(c->weigh_wide_wgs > 0 ? (uint32_t)c->weigh_wide_wgs : cus, kWideMaxWgs);
        const uint32_t slab_rows = n_wg + n_buckets;
        const size_t room = (size_t)wide_room(n);
        const size_t plan_bytes = (sizeof(WidePlan) + 127) & ~(size_t)127;
        HIP_TRY(c, c->w_wide.reserve(room * 4));
        HIP_TRY(c, c->w_wide_plan.reserve(plan_bytes + 1024 + (size_t)kWideMaxBuckets * kWideCursorPad * 4));
        HIP_TRY(c, c->w_slab.reserve((size_t)slab_rows * kSliceBins * 4));
        WidePlan* plan = reinterpret_cast<WidePlan*>(c->w_wide_plan.p);
        uint32_t* bucket_count = reinterpret_cast<uint32_t*>(static_cast<char*>(c->w_wide_plan.p) + plan_bytes);
        uint32_t* cursor = bucket_count + 256;
        HIP_TRY(c, hipMemsetAsync(bucket_count, 0, 1024, c->stream));
        const uint32_t n_tiles = (n + kWideTile - 1u) / kWideTile;
        const dim3 pgrid(std::max(1u, std::min(n_tiles, 2u * cus)));
        kt = ktimer_begin(c, "weigh_wide_part");
        hipLaunchKernelGGL(wide_count_kernel, pgrid, dim3(kWideThreads), 0, c->stream, one_words, n, n_buckets, bucket_count);
        hipLaunchKernelGGL(wide_scan_kernel, dim3(1), dim3(256), 0, c->stream, bucket_count, n_buckets, n_wg, plan, cursor);
        hipLaunchKernelGGL(wide_scatter_kernel, pgrid, dim3(kWideThreads), 0, c->stream, one_words, n, n_buckets, cursor,
                           c->w_wide.as<uint32_t>(), (uint32_t)std::min<size_t>(room, 0xFFFFFFFFu));
        ktimer_end(c, kt);
        WideBinsArgs wa{};
        wa.words = c->w_wide.as<uint32_t>();
        wa.plan = plan;
        wa.n_subjects = (uint32_t)c->n_subjects;
        wa.slab = c->w_slab.as<uint32_t>();
        wa.slab_rows = slab_rows;
        wa.hi = c->w_hi.as<uint32_t>();
        wa.err = scalar_err(c);
        kt = ktimer_begin(c, "weigh_wide");
        hipLaunchKernelGGL((weigh_wide_kernel<4>), dim3(n_wg), dim3(kWeighThreads), kBinsMaxLds, c->stream, wa);
        ktimer_end(c, kt);
        wm.slab = wa.slab;
        wm.hi = wa.hi;
        wm.wide_first = plan->item_first;
        wm.bins = kSliceBins;
        wm.n_teams = 0;
    } else {
        // ---- more slices than streams: one stream, a team of workgroups per tile (round 3's launch)
        uint32_t w_xcd = 8;
        if (cus % w_xcd) w_xcd = 1;
        const int64_t cap = (int64_t)kBinsMaxLds / 4 - 96;
        const uint32_t w_slices = (uint32_t)((c->n_subjects + cap - 1) / cap);
        const uint32_t w_bins = ((uint32_t)c->n_subjects + w_slices - 1) / w_slices;
        const uint32_t w_teams = words_team_size(c);
        const uint32_t n_teams = w_xcd * w_teams;
        HIP_TRY(c, c->w_slab.reserve((size_t)w_slices * n_teams * w_bins * 4));
        BinsArgs ba{};
        ba.subj = reinterpret_cast<const int32_t*>(one_words);
        ba.rk = nullptr;
        ba.n_records = (uint32_t)one_count;
        ba.n_subjects = (uint32_t)c->n_subjects;
        ba.bins = w_bins;
        ba.n_slices = w_slices;
        ba.teams_per_xcd = w_teams;
        ba.n_xcd = w_xcd;
        ba.slab = c->w_slab.as<uint32_t>();
        ba.hi = c->w_hi.as<uint32_t>();
        ba.err = scalar_err(c);
        const dim3 wgrid(cus);
        const size_t wlds = ((size_t)w_bins + 96) * 4;
        kt = ktimer_begin(c, "classify");
        if (c->bins_ring == 6)
            hipLaunchKernelGGL((weigh_bins_kernel<6, true>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
        else if (c->bins_ring == 8)
            hipLaunchKernelGGL((weigh_bins_kernel<8, true>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
        else
            hipLaunchKernelGGL((weigh_bins_kernel<4, true>), wgrid, dim3(kWeighThreads), wlds, c->stream, ba);
        ktimer_end(c, kt);
        wm.slab = ba.slab;
        wm.hi = ba.hi;
        wm.bins = w_bins;
        wm.n_teams = n_teams;
    }
    kt = ktimer_begin(c, "weigh_merge");
    wm.n_subjects = (uint32_t)c->n_subjects;
    // (a subject table that grew past the streams' slices since they were opened -- past kMaxStreams slices: the
    // accumulation is flushed by `words_roll` and goes on unsliced -- holds no records of the subjects behind them; the
    // merge stops at the last stream's slice, its rows are all there are)
    if (wm.streams) wm.n_subjects = (uint32_t)std::min<int64_t>(c->n_subjects, (int64_t)wm.streams * kSliceBins);
    wm.rows = a.rows;
    wm.row_w = a.row_w;
    wm.n_jobs = n_jobs;
    for (int j = 0; j < n_jobs; ++j) {
        wm.mode[j] = a.jobs[j].mode;
        wm.col[j] = a.jobs[j].col;
        wm.job_id[j] = job_id[j];
    }
    wm.group = (uint32_t)c->w_group;
    wm.table = CountTable{c->tkeys.as<unsigned long long>(), c->tvals.as<unsigned long long>(), c->slots - 1, scalar_err(c)};
    hipLaunchKernelGGL(weigh_merge_kernel, dim3((wm.n_subjects + kMergeSubjects - 1u) / kMergeSubjects), dim3(1024), (size_t)4096 * 16, c->stream, wm, 4096u);
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    if (!mixed) {  // (a mixed set: counted by its first whole-read job)
        c->stat_extra_reads += c->w_reads;
        c->stat_extra_records += c->w_records;
    }
    if (c->words_keep) return WK_OK;  // (bench: repeated passes over the resident batch)
    return words_reset(c);
}

static int words_begin(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t group, int* ok, bool mixed) {
    if (!c || !ok) return WK_E_ARG;
    *ok = 0;
    if (!jobs || n_jobs < 1 || n_jobs > WK_MAX_JOBS) return fail(c, WK_E_ARG, "n_jobs must be in [1,%d]", WK_MAX_JOBS);
    if (group < 0 || group >= (1 << WK_KEY_GROUP_BITS)) return fail(c, WK_E_ARG, "group id outside [0, %d)", 1 << WK_KEY_GROUP_BITS);
    DeviceGuard guard(c->device);
    // records accumulated under other jobs / another group are classified first
    if (c->w_open && c->w_records > 0 && (group != c->w_group || !same_jobs(c->w_jobs, jobs, n_jobs))) {
        const int rc = wk_words_flush(c);
        if (rc) return rc;
    }
    ClassifyArgs a{};
    bool good = false;
    int mode = 0;
    int rc = words_jobs_ok(c, jobs, n_jobs, a, &good, &mode, mixed);
    if (rc) return rc;
    if (!good) {
        // (what is there was appended while every subject was valid: classify it now)
        if (c->w_open && c->w_records > 0 && (rc = wk_words_flush(c))) return rc;
        c->w_open = false;
        return WK_OK;
    }
    if (!c->w_open || c->w_records == 0) {  // a fresh accumulation
        if ((rc = words_reset(c))) return rc;
        c->w_sliced = mode == 0 && c->use_streams && !c->weigh_wide && streams_needed(c) <= kMaxStreams;
        c->w_streams = 0;
    }
    c->w_jobs.assign(jobs, jobs + n_jobs);
    c->w_group = group;
    c->w_mode = mode;
    c->w_mixed_entry = mixed;
    c->w_open = true;
    *ok = 1;
    return WK_OK;
}

int wk_words_begin(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t group, int* ok) {
    return words_begin(c, jobs, n_jobs, group, ok, false);
}

int wk_words_begin_mixed(wk_ctx* c, const wk_job* jobs, int32_t n_jobs, int32_t group, int* ok) {
    return words_begin(c, jobs, n_jobs, group, ok, true);
}

static StreamSet stream_set(wk_ctx* c) {
    StreamSet s{};
    size_t cap = ~(size_t)0;
    for (int k = 0; k < c->w_streams; ++k) {
        s.out[k] = c->w_stream[k].as<uint32_t>();
        cap = std::min(cap, c->w_stream[k].cap / 4);
    }
    s.cursor = c->w_cursor.as<unsigned long long>();
    s.n_streams = (uint32_t)c->w_streams;
    s.cap = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu);
    return s;
}

// Single-job accumulation of the per-read stream: the first `count` records name their nodes by rank among the
// subjects' nodes.  When the subject table has grown since they were written, they are renumbered.
static int refresh_word_ranks(wk_ctx* c, int64_t count) {
    wk_ctx::StreamTables& T = c->st[0];
    std::vector<int32_t> before;
    const int rc = ensure_rank_table(c, T, c->w_mode, c->w_mode == 2 ? c->w_jobs[0].rank_slot : -1, &before);
    if (rc) return rc;
    if (count <= 0 || before.empty() || before == T.dn_host) return WK_OK;
    std::vector<int32_t> new_of_old(before.size());
    for (size_t i = 0; i < before.size(); ++i) {
        const auto it = std::lower_bound(T.dn_host.begin(), T.dn_host.end(), before[i]);
        if (it == T.dn_host.end() || *it != before[i]) return fail(c, WK_E_STATE, "a subject changed its node under accumulated records");
        new_of_old[i] = (int32_t)(it - T.dn_host.begin());
    }
    const int rcu = upload(c, c->w_renum, new_of_old.data(), new_of_old.size() * 4);
    if (rcu) return rcu;
    hipLaunchKernelGGL(ranks_renumber_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, c->c_words.as<uint32_t>(),
                       (uint32_t)count, c->w_renum.as<int32_t>(), (uint32_t)before.size());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the vector is about to go out of scope)
    return WK_OK;
}

// ... and the subject fields of words [first, first + n), subject indices as the tokenizers write them, become such ranks.
static int words_translate(wk_ctx* c, int64_t first, int64_t n) {
    if ((c->w_mode != 1 && c->w_mode != 2) || n <= 0) return WK_OK;  // (several stream jobs: rewritten per job at the flush)
    const int rc = refresh_word_ranks(c, first);
    if (rc) return rc;
    hipLaunchKernelGGL(words_to_ranks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       c->c_words.as<uint32_t>() + first, c->c_words.as<uint32_t>() + first, (uint32_t)n,
                       c->st[0].subj_rank.as<int32_t>(), (uint32_t)c->n_subjects, scalar_err(c));
    HIP_TRY(c, hipGetLastError());
    return WK_OK;
}

// Room for n_more records behind the accumulated ones.
static int words_room(wk_ctx* c, int64_t n_more) {
    if (c->w_mode == 0) {
        // every stream may take all of them (its cursor is only known to the device: at most w_records)
        if (!c->w_cursor.p) {
            HIP_TRY(c, c->w_cursor.reserve(kMaxStreams * 8));
            HIP_TRY(c, hipMemsetAsync(c->w_cursor.p, 0, kMaxStreams * 8, c->stream));
        }
        const int want = c->w_sliced ? streams_needed(c) : 1;
        c->w_streams = std::max(c->w_streams, want);
        const size_t need = (size_t)(c->w_records + n_more) * 4 + 64;
        const size_t room = std::max(need * 2, (size_t)std::max<int64_t>(c->w_expect, 0) * 4 + 64);
        for (int k = 0; k < c->w_streams; ++k) {
            DevBuf& b = c->w_stream[k];
            if (need <= b.cap) continue;
            DevBuf bigger;
            HIP_TRY(c, bigger.reserve(room));
            const size_t keep = std::min((size_t)c->w_records * 4, b.cap);
            if (keep > 0) HIP_TRY(c, hipMemcpyAsync(bigger.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            b.release();
            b = bigger;
        }
        return WK_OK;
    }
    const size_t need = (size_t)(c->w_records + n_more) * 4 + 64;
    if (need <= c->c_words.cap) return WK_OK;
    // grow: a new buffer (twice the need, or what the sample is expected to bring) takes over what is there
    DevBuf bigger;
    HIP_TRY(c, bigger.reserve(std::max(need * 2, (size_t)std::max<int64_t>(c->w_expect, 0) * 4 + 64)));
    if (c->w_records > 0) HIP_TRY(c, hipMemcpyAsync(bigger.p, c->c_words.p, (size_t)c->w_records * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->c_words.release();
    c->c_words = bigger;
    return WK_OK;
}

// The accumulated records would pass 2^30 (the histogram addresses bytes with
// 32 bits): classify what is there and open the same job set again.
static int words_roll(wk_ctx* c, int64_t n_more) {
    const bool outgrown = c->w_mode == 0 && c->w_sliced && streams_needed(c) > kMaxStreams;  // (continues unsliced)
    if (c->w_records + n_more < (1ll << 30) && !outgrown) return WK_OK;
    const std::vector<wk_job> jobs = c->w_jobs;
    const int32_t group = c->w_group;
    const bool mixed = c->w_mixed_entry;  // (re-opened through the gate that opened it)
    int rc = wk_words_flush(c);
    if (rc) return rc;
    int ok = 0;
    if ((rc = words_begin(c, jobs.data(), (int32_t)jobs.size(), group, &ok, mixed))) return rc;
    if (!ok) return fail(c, WK_E_STATE, "job set no longer accepted");
    if (n_more >= (1ll << 30)) return fail(c, WK_E_RANGE, "more than 2^30 records in one block");
    return WK_OK;
}

int wk_words_append(wk_ctx* c, const uint32_t* words, int64_t n_records, int64_t n_reads, int slot) {
    if (!c) return WK_E_ARG;
    if (n_records < 0 || n_reads < 0 || (n_records > 0 && !words)) return fail(c, WK_E_ARG, "bad packed record arguments");
    if (!c->w_open) return fail(c, WK_E_STATE, "wk_words_begin has not accepted a job set");
    if (c->lag_count) return fail(c, WK_E_STATE, "blocks whose verdict has not been read (wk_dtok_scan_emit_end)");
    c->fz_chain = false;
    if (slot < -1 || slot >= wk_ctx::kStageSlots) return fail(c, WK_E_ARG, "slot must be -1 or in [0, %d)", wk_ctx::kStageSlots);
    DeviceGuard guard(c->device);
    {
        const int rcr = words_roll(c, n_records);
        if (rcr) return rcr;
    }
    {
        const int rcw = words_room(c, n_records);
        if (rcw) return rcw;
    }
    if (n_records > 0 && c->w_mode == 0) {
        HIP_TRY(c, c->w_stage.reserve((size_t)n_records * 4));
        HIP_TRY(c, hipMemcpyAsync(c->w_stage.p, words, (size_t)n_records * 4, hipMemcpyHostToDevice, c->stream));
    } else if (n_records > 0) {
        HIP_TRY(c, hipMemcpyAsync(c->c_words.as<uint32_t>() + c->w_records, words, (size_t)n_records * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (slot >= 0) {
        if (!c->slot_ev[slot]) HIP_TRY(c, hipEventCreateWithFlags(&c->slot_ev[slot], hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->slot_ev[slot], c->stream));
        c->slot_busy[slot] = true;
    }
    if (n_records > 0 && c->w_mode == 0) {  // ... to the streams of their slices
        hipLaunchKernelGGL(words_partition_kernel, dim3((unsigned)((n_records + 256 * kScatterItems - 1) / (256 * kScatterItems))), dim3(256), 0, c->stream,
                           c->w_stage.as<uint32_t>(), (uint32_t)n_records, stream_set(c));
        HIP_TRY(c, hipGetLastError());
        c->w_counts_known = false;
    }
    {
        const int rct = words_translate(c, c->w_records, n_records);
        if (rct) return rct;
    }
    if (slot < 0) HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's buffer is only valid during the call
    c->w_records += n_records;
    c->w_reads += n_reads;
    return WK_OK;
}

int wk_words_wait(wk_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= wk_ctx::kStageSlots) return WK_E_ARG;
    if (!c->slot_busy[slot]) return WK_OK;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipEventSynchronize(c->slot_ev[slot]));
    c->slot_busy[slot] = false;
    return WK_OK;
}

int wk_words_pending(wk_ctx* c, int64_t* n_records, int64_t* n_reads) {
    if (!c) return WK_E_ARG;
    if (n_records) *n_records = c->w_open ? c->w_records : 0;
    if (n_reads) *n_reads = c->w_open ? c->w_reads : 0;
    return WK_OK;
}

// ---- SAM tokenizer on the device --------------------------------------------------

// The dictionary of `tok` as the kernels probe it: open addressing, 16-byte slots
// {hash, id, offset}, the names behind 4-byte lengths in one arena.
static int dtok_mirror_dict(wk_ctx* c, const wk_tok* tok) {
    const int32_t n = wkx_tok_n_names(tok);
    if (c->dt_dict_tok == tok && c->dt_dict_names == n) return WK_OK;
    uint32_t slots = 1024;
    while (slots < 2u * (uint32_t)n + 2u) slots <<= 1;
    std::vector<DictSlot> tab(slots, DictSlot{0ull, -1, 0u});
    std::string arena;
    arena.reserve((size_t)n * 16 + 16);
    for (int32_t id = 0; id < n; ++id) {
        const char* p;
        uint32_t len;
        uint64_t hv;
        wkx_tok_name(tok, id, &p, &len, &hv);
        const uint32_t off = (uint32_t)arena.size();
        arena.append(reinterpret_cast<const char*>(&len), 4);
        arena.append(p, len);
        uint32_t h = (uint32_t)hv & (slots - 1);
        while (tab[h].id >= 0) h = (h + 1) & (slots - 1);
        tab[h] = DictSlot{(unsigned long long)hv, id, off};
    }
    arena.append(16, '\0');
    int rc;
    if ((rc = upload(c, c->d_dict, tab.data(), tab.size() * sizeof(DictSlot)))) return rc;
    if ((rc = upload(c, c->d_arena, arena.data(), arena.size()))) return rc;
    // (the same table for dtok_fused_kernel: 8-byte slots, the names by id)
    std::vector<DictSlot8> tab8(slots, DictSlot8{0u, -1});
    std::vector<unsigned char> names16((size_t)std::max(n, 1) * 16, 0);
    for (uint32_t h = 0; h < slots; ++h) {
        if (tab[h].id < 0) continue;
        tab8[h] = DictSlot8{(uint32_t)(tab[h].hash >> 32), tab[h].id};
        uint32_t len;
        std::memcpy(&len, arena.data() + tab[h].off, 4);
        unsigned char* rec = names16.data() + (size_t)tab[h].id * 16;
        if (len <= 15) {
            std::memcpy(rec, arena.data() + tab[h].off + 4, len);
            rec[15] = (unsigned char)len;
        } else {
            std::memcpy(rec, &tab[h].off, 4);
            rec[15] = 0xFF;
        }
    }
    if ((rc = upload(c, c->d_dict2, tab8.data(), tab8.size() * sizeof(DictSlot8)))) return rc;
    if ((rc = upload(c, c->d_names16, names16.data(), names16.size()))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->dt_dict_mask = slots - 1;
    c->dt_dict_names = n;
    c->dt_dict_tok = tok;
    return WK_OK;
}

static DtokArgs dtok_args(wk_ctx* c) {
    DtokArgs a{};
    a.text = c->dt_text;
    a.n = c->dt_n;
    a.fmt = (uint32_t)c->dt_fmt;
    a.line_start = c->d_lines.as<uint32_t>();
    a.n_lines = c->dt_lines;
    a.lsubj = c->d_lsubj.as<int32_t>();
    a.lmeta = c->d_lmeta.as<uint32_t>();
    a.dict = c->d_dict.as<DictSlot>();
    a.dict_mask = c->dt_dict_mask;
    a.arena = c->d_arena.as<unsigned char>();
    a.dict8 = c->d_dict2.as<DictSlot8>();
    a.names16 = c->d_names16.as<uint4>();
    a.unknown = c->d_unknown.as<uint2>();
    a.unknown_cap = (uint32_t)(c->d_unknown.cap / 8);
    a.is_start = c->d_start.as<unsigned char>();
    a.is_first = c->d_first.as<unsigned char>();
    a.state = c->d_state.as<DtokState>();
    a.lbeg = c->d_lbeg.as<int32_t>();
    a.lend = c->d_lend.as<int32_t>();
    a.llen = c->d_llen.as<uint32_t>();
    a.line_scan = c->d_lscan.as<unsigned long long>();
    a.submap = c->dt_submap_on ? c->d_submap.as<int32_t>() : nullptr;
    a.n_submap = c->dt_submap_n;
    return a;
}

// Newlines of text[0, n) per tile of kDtokTile bytes into tiles[], their exclusive prefix sums into tile_off[], the
// total to *total (device or pinned memory) -- queued on `stream`.  The count zeroes the 64 bytes of pad behind the text.
static void count_newlines(const unsigned char* text, uint32_t n, unsigned long long* tiles, unsigned long long* tile_off,
                           unsigned long long* total, hipStream_t stream) {
    const uint32_t n_tiles = (n + kDtokTile - 1) / kDtokTile;
    hipLaunchKernelGGL(dtok_count_kernel, dim3(n_tiles), dim3(kDtokThreads), 0, stream, text, n, tiles);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, stream, tiles, tile_off, (int64_t)n_tiles, total);
}

// hipMemcpyAsync host -> device of [src, src + n), cut where registered ranges
// (wk_host_register) begin and end: one copy may not span two registrations.
static hipError_t copy_text_async(wk_ctx* c, void* dst, const char* src, size_t n, hipStream_t stream) {
    std::vector<size_t> cuts{0, n};
    {
        std::lock_guard<std::mutex> lock(c->reg_mu);
        for (const wk_ctx::HostReg& r : c->regs) {
            if (r.p > src && r.p < src + n) cuts.push_back((size_t)(r.p - src));
            if (r.p + r.n > src && r.p + r.n < src + n) cuts.push_back((size_t)(r.p + r.n - src));
        }
    }
    std::sort(cuts.begin(), cuts.end());
    for (size_t i = 0; i + 1 < cuts.size(); ++i) {
        if (cuts[i + 1] == cuts[i]) continue;
        const hipError_t e = hipMemcpyAsync((char*)dst + cuts[i], src + cuts[i], cuts[i + 1] - cuts[i], hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int wk_host_register(wk_ctx* c, const void* p, size_t bytes) {
    if (!c || !p || !bytes) return WK_E_ARG;
    DeviceGuard guard(c->device);
    const hipError_t e = hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterReadOnly);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, WK_E_HIP, "hipHostRegister(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lock(c->reg_mu);
    c->regs.push_back(wk_ctx::HostReg{(const char*)p, bytes});
    return WK_OK;
}

int wk_host_unregister(wk_ctx* c, const void* p) {
    if (!c || !p) return WK_E_ARG;
    {
        std::lock_guard<std::mutex> lock(c->reg_mu);
        auto it = std::find_if(c->regs.begin(), c->regs.end(), [&](const wk_ctx::HostReg& r) { return r.p == (const char*)p; });
        if (it == c->regs.end()) return fail(c, WK_E_ARG, "not a registered range");
        c->regs.erase(it);
    }
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipHostUnregister(const_cast<void*>(p)));
    return WK_OK;
}

static int dinf_check_spans(wk_ctx* c, int64_t n_blob, const int64_t* lo, const int64_t* hi, const int64_t* off, int64_t n);
static void dinf_launch(wk_ctx* c, const unsigned char* d_blob, const int64_t* d_meta, int64_t n, unsigned char* d_out, uint32_t* d_status,
                        hipStream_t s);

// (wk_dtok_inflate_ahead) what a block is made of when its text is inflated on the device instead of copied
struct DinfAhead {
    int64_t n_comp;
    const int64_t *lo, *hi, *off;
    int64_t n_members;
    const char* carry;
    int64_t n_carry;
    char last;
};

static int dtok_copy_impl(wk_ctx* c, const char* text, int64_t begin, int64_t stop, bool detached, int32_t* ticket,
                          const DinfAhead* inf = nullptr) {
    if (!c || !text || begin < 0 || stop < begin) return WK_E_ARG;
    if (ticket) *ticket = -1;
    Lap lap(&c->lap_s[0]);
    const int64_t n64 = stop - begin;
    if (n64 == 0 || n64 >= (1ll << 31) - 64) return WK_OK;
    auto lap_t = std::chrono::steady_clock::now();
    DeviceGuard guard(c->device);
    int k = -1;
    {
        std::lock_guard<std::mutex> lock(c->copy_mu);
        if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->count_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->count_stream, hipStreamNonBlocking));
        k = textbuf_take_free(c, wk_ctx::kBufCopied);  // (tagged below, once the copy is queued)
        if (k >= 0) c->text_buf[k].seq = c->copy_seq_next++;
    }
    if (k < 0) return fail(c, WK_E_STATE, "more than %d blocks copied ahead of the scan", wk_ctx::kTextBufs - 1);
    TextBuf& b = c->text_buf[k];
    auto lap_mark = [&](int i) {
        const auto now = std::chrono::steady_clock::now();
        const double dt = std::chrono::duration<double>(now - lap_t).count();
        c->lap_c[i] += dt;
        if (i == 1) c->lap_c[4] = std::max(c->lap_c[4], dt);
        lap_t = now;
    };
    if (!b.ev) HIP_TRY(c, hipEventCreate(&b.ev));
    if (!b.ev0) HIP_TRY(c, hipEventCreate(&b.ev0));
    if (!b.evm) HIP_TRY(c, hipEventCreate(&b.evm));
    const uint32_t n = (uint32_t)n64;
    // (at least a full block's worth from the start: a file's first blocks are small, and growing a buffer
    // three times means three hipFree / hipMalloc pairs per buffer while the dictionary is cold)
    lap_mark(0);
    HIP_TRY(c, text_buffer(c, k, (inf ? (size_t)(inf->n_carry + inf->off[inf->n_members]) : (size_t)n) + 64));
    lap_mark(1);
    HIP_TRY(c, hipEventRecord(b.ev0, c->copy_stream));
    b.di_used = inf != nullptr;
    if (inf) {
        // the carry, then the members' text behind it: compressed bytes and spans in, one launch of the inflate
        // kernel, its failure word out to pinned memory -- all on the copy stream, so the scan of the block before
        // goes on meanwhile.  (Spans and carry are the caller's for this call only: the copies read this buffer's own.)
        const int64_t nm = inf->n_members;
        if (!c->di_any_host) HIP_TRY(c, hipHostMalloc((void**)&c->di_any_host, sizeof(uint32_t) * wk_ctx::kTextBufs, hipHostMallocDefault));
        HIP_TRY(c, b.di_comp.reserve((size_t)inf->n_comp));
        HIP_TRY(c, b.di_meta.reserve((size_t)(3 * nm + 1) * 8));
        HIP_TRY(c, b.di_status.reserve((size_t)(nm + 2) * 4));
        std::vector<int64_t>& meta = b.di_meta_host;
        meta.resize((size_t)(3 * nm + 1));
        std::copy(inf->lo, inf->lo + nm, meta.begin());
        std::copy(inf->hi, inf->hi + nm, meta.begin() + nm);
        for (int64_t i = 0; i <= nm; ++i) meta[(size_t)(2 * nm + i)] = inf->off[i] + inf->n_carry;
        b.di_carry_host.assign(inf->carry, inf->carry + inf->n_carry);
        int64_t* d_meta = b.di_meta.as<int64_t>();
        c->di_any_host[k] = 0;
        if (inf->n_carry)
            HIP_TRY(c, hipMemcpyAsync(b.text, b.di_carry_host.data(), (size_t)inf->n_carry, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(c, hipMemcpyAsync(b.di_comp.p, text, (size_t)inf->n_comp, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(c, hipMemcpyAsync(d_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(c, hipMemsetAsync(b.di_status.p, 0, (size_t)(nm + 2) * 4, c->copy_stream));
        dinf_launch(c, b.di_comp.as<unsigned char>(), d_meta, nm, b.text, b.di_status.as<uint32_t>(), c->copy_stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&c->di_any_host[k], b.di_status.as<uint32_t>() + nm, 4, hipMemcpyDeviceToHost, c->copy_stream));
    } else {
        // (only the copy on this stream: the 64 zero bytes behind the text are written by the newline count,
        // which runs on another stream behind the copy's event -- here or in the scan)
        HIP_TRY(c, copy_text_async(c, b.text, text + begin, (size_t)n, c->copy_stream));
    }
    HIP_TRY(c, hipEventRecord(b.evm, c->copy_stream));
    lap_mark(2);
    // ... and, behind the copy, the count of the block's newlines -- on a stream of its own, so that the next
    // block's copy follows this one without a gap; the total lands in pinned memory (written by the kernel: no
    // trip through the DMA queue): wk_dtok_scan finds the number on the host instead of waiting for it
    HIP_TRY(c, hipStreamWaitEvent(c->count_stream, b.evm, 0));
    b.counted = false;
    if (!c->fused_streak && c->count_ahead) {  // (blocks that go through the one kernel need no count: wk_dtok_fused.hpp)
        const uint32_t n_tiles = (n + kDtokTile - 1) / kDtokTile;
        HIP_TRY(c, b.tiles.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, b.tile_off.reserve((size_t)n_tiles * 8));
        count_newlines(b.text, n, b.tiles.as<unsigned long long>(), b.tile_off.as<unsigned long long>(), &c->copy_newlines[k],
                       c->count_stream);
        HIP_TRY(c, hipGetLastError());
        b.counted = true;
    }
    HIP_TRY(c, hipEventRecord(b.ev, c->count_stream));
    lap_mark(3);
    {
        // (the tag last: from here on a scan finds the block, on whatever thread it runs)
        std::lock_guard<std::mutex> lock(c->copy_mu);
        b.n = n;
        b.last = inf ? inf->last : text[stop - 1];
        b.detached = detached;
        b.src = text + begin;
    }
    if (ticket) *ticket = k;
    return WK_OK;
}

int wk_dtok_copy(wk_ctx* c, const char* text, int64_t begin, int64_t stop) {
    return dtok_copy_impl(c, text, begin, stop, false, nullptr);
}

// The same copy for a reader that does not keep the host bytes until the block is scanned: `ticket` names the copy for
// wk_dtok_copy_wait, after which text[begin, stop) may be overwritten.  The scan of the block is called with the same
// (text, begin, stop) as ever -- the pointer is only the block's tag then; where it wants the bytes themselves (names
// of subjects the dictionary does not hold) they are fetched from the device, and wk_dtok_text_back hands the host
// layer the block's text when the kernels leave the block to the host tokenizer.
int wk_dtok_copy_ahead(wk_ctx* c, const char* text, int64_t begin, int64_t stop, int32_t* ticket) {
    if (!ticket) return WK_E_ARG;
    return dtok_copy_impl(c, text, begin, stop, true, ticket);
}

int wk_dtok_copy_wait(wk_ctx* c, int32_t ticket) {
    if (!c) return WK_E_ARG;
    if (ticket < 0) return WK_OK;  // (an empty block: nothing was copied)
    if (ticket >= wk_ctx::kTextBufs || !c->text_buf[ticket].evm) return fail(c, WK_E_ARG, "not a ticket of wk_dtok_copy_ahead");
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipEventSynchronize(c->text_buf[ticket].evm));
    if (c->text_buf[ticket].di_used && c->di_any_host && c->di_any_host[ticket])
        return fail(c, WK_E_STATE, "gzip member: one of the block does not inflate to what its trailer says (stream, size, CRC-32)");
    return WK_OK;
}

// The sibling of wk_dtok_copy_ahead for gzip members that state their size: the next text buffer is filled with
// carry[0, n_carry) followed by the text of the members, inflated there (wk_dinflate.hpp), and [0, stop) of it is the
// block that the scan tagged (comp, 0, stop) finds.  What lies behind `stop` in the buffer is not part of the block.
int wk_dtok_inflate_ahead(wk_ctx* c, const char* comp, int64_t n_comp, const int64_t* lo, const int64_t* hi, const int64_t* off,
                          int64_t n_members, const char* carry, int64_t n_carry, int64_t begin, int64_t stop, int last_byte,
                          int32_t* ticket) {
    if (!c || !comp || n_comp <= 0 || !lo || !hi || !off || n_members <= 0 || n_members >= (1ll << 31) || n_carry < 0 || (n_carry && !carry) ||
        !ticket)
        return WK_E_ARG;
    if (begin != 0) return fail(c, WK_E_ARG, "a block inflated on the device begins with its buffer (begin = %lld)", (long long)begin);
    if (int rc = dinf_check_spans(c, n_comp, lo, hi, off, n_members)) return rc;
    if (stop <= 0 || stop > n_carry + off[n_members]) return fail(c, WK_E_ARG, "the block ends outside its text");
    const DinfAhead inf{n_comp, lo, hi, off, n_members, carry, n_carry, (char)last_byte};
    return dtok_copy_impl(c, comp, 0, stop, true, ticket, &inf);
}

// The text blocks scanned from now on belong to `text_bytes` bytes of one sample (0: unknown again): the buffers of its
// records are sized for all of them when the first block is emitted.
int wk_dtok_expect(wk_ctx* c, int64_t text_bytes) {
    if (!c || text_bytes < 0) return WK_E_ARG;
    c->dt_expect_bytes = text_bytes;
    c->w_expect = 0;
    return WK_OK;
}

// Forget the blocks copied ahead that no scan has asked for (the file goes another way after all).
int wk_dtok_copy_drop(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    if (c->count_stream) HIP_TRY(c, hipStreamSynchronize(c->count_stream));
    std::lock_guard<std::mutex> lock(c->copy_mu);
    for (int q = 0; q < wk_ctx::kTextBufs; ++q)
        if (c->text_buf[q].state == wk_ctx::kBufCopied) textbuf_claim(c, q, wk_ctx::kBufFree);
    for (TextBuf& b : c->text_buf)
        if (b.state == wk_ctx::kBufFree)   // (compressed bytes of blocks long scanned)
            for (DevBuf* d : {&b.di_comp, &b.di_meta, &b.di_status}) d->release();
    // (the slabs a reader far ahead of the scans took -- up to 12 GB -- go back to the device once none of their
    // buffers is in use: what follows the file, count tables and records, must not compete with parked text.
    // The first slab stays: a reader that keeps close to the scans lives in it)
    {
        std::lock_guard<std::mutex> slabs(c->slab_mu);
        for (int sl = 1; sl < wk_ctx::kTextBufs / wk_ctx::kSlabBufs; ++sl) {
            if (!c->d_textslab[sl].p) continue;
            bool idle = true;
            for (int q = sl * wk_ctx::kSlabBufs; q < (sl + 1) * wk_ctx::kSlabBufs; ++q) idle = idle && c->text_buf[q].state == wk_ctx::kBufFree;
            if (!idle) continue;
            HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the scan of a block that lived there)
            for (int q = sl * wk_ctx::kSlabBufs; q < (sl + 1) * wk_ctx::kSlabBufs; ++q)
                if (c->text_buf[q].text >= c->d_textslab[sl].as<unsigned char>() &&
                    c->text_buf[q].text < c->d_textslab[sl].as<unsigned char>() + wk_ctx::kTextStride * wk_ctx::kSlabBufs)
                    c->text_buf[q].text = nullptr;
            if (c->dt_text >= c->d_textslab[sl].as<unsigned char>() && c->dt_text < c->d_textslab[sl].as<unsigned char>() + c->d_textslab[sl].cap)
                c->dt_text = nullptr;  // (wk_dtok_text_back of that block: refused from now on)
            c->d_textslab[sl].release();
        }
    }
    return WK_OK;
}

// How many blocks a reader may copy ahead of the scans on this device as it is now: half of the memory that is free
// (slabs already taken for text count as free: they are reused), in text buffers of one block each.
int wk_dtok_ahead_room(wk_ctx* c, int32_t* n_blocks) {
    if (!c || !n_blocks) return WK_E_ARG;
    DeviceGuard guard(c->device);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    size_t held = 0;
    {
        std::lock_guard<std::mutex> slabs(c->slab_mu);
        for (const DevBuf& b : c->d_textslab) held += b.p ? b.cap : 0;
    }
    const size_t room = (free_b + held) / 2 / wk_ctx::kTextStride;
    *n_blocks = (int32_t)std::min<size_t>(room, (size_t)wk_ctx::kTextBufs - 1);
    return WK_OK;
}

// The text of the block scanned last, as the device holds it: n = stop - begin bytes into `out`.
int wk_dtok_text_back(wk_ctx* c, char* out, int64_t n) {
    if (!c || !out || n < 0) return WK_E_ARG;
    if (!c->dt_text || (int64_t)c->dt_n != n) return fail(c, WK_E_STATE, "no scanned block of %lld bytes on the device", (long long)n);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(out, c->dt_text, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// ---- gzip members inflated on the device (wk_dinflate.hpp) ---------------------------------------
// Spans that the kernel may be given: streams inside the blob with room for a trailer, sizes that fit 31 bits.
static int dinf_check_spans(wk_ctx* c, int64_t n_blob, const int64_t* lo, const int64_t* hi, const int64_t* off, int64_t n) {
    if (off[0] != 0) return fail(c, WK_E_ARG, "off[0] is not 0");
    for (int64_t i = 0; i < n; ++i) {
        if (lo[i] < 0 || hi[i] > n_blob || hi[i] - lo[i] < 8 || hi[i] - lo[i] >= (1ll << 31))
            return fail(c, WK_E_ARG, "member %lld: compressed span [%lld, %lld) is not inside the %lld bytes given", (long long)i,
                        (long long)lo[i], (long long)hi[i], (long long)n_blob);
        if (off[i + 1] < off[i] || off[i + 1] - off[i] >= (1ll << 31))
            return fail(c, WK_E_ARG, "member %lld: a size of %lld bytes", (long long)i, (long long)(off[i + 1] - off[i]));
    }
    return WK_OK;
}

// d_meta: lo[n], hi[n], off[n + 1]; d_status: n words, then "any failed" and the hand-out counter
static void dinf_launch(wk_ctx* c, const unsigned char* d_blob, const int64_t* d_meta, int64_t n, unsigned char* d_out, uint32_t* d_status,
                        hipStream_t s) {
    const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)c->prop.multiProcessorCount * kDinfWavesPerCu);
    hipLaunchKernelGGL(dinflate_kernel, dim3(grid), dim3(64), 0, s, d_blob, d_meta, d_meta + n, d_meta + 2 * n, (uint32_t)n, d_out, d_status,
                       d_status + n, d_status + n + 1);
}

int wk_inflate_members_device(wk_ctx* c, const char* blob, int64_t n_blob, const int64_t* lo, const int64_t* hi, const int64_t* off, int64_t n,
                              char* out, uint32_t* status) {
    if (!c || !blob || n_blob <= 0 || !lo || !hi || !off || n <= 0 || n >= (1ll << 31) || !status) return WK_E_ARG;
    if (int rc = dinf_check_spans(c, n_blob, lo, hi, off, n)) return rc;
    const int64_t total = off[n];
    if (total && !out) return WK_E_ARG;
    DeviceGuard guard(c->device);
    constexpr size_t kGuard = 256;
    HIP_TRY(c, c->di_blob.reserve((size_t)n_blob));
    HIP_TRY(c, c->di_meta.reserve((size_t)(3 * n + 1) * 8));
    HIP_TRY(c, c->di_out.reserve((size_t)total + 2 * kGuard));
    HIP_TRY(c, c->di_status.reserve((size_t)(n + 2) * 4));
    unsigned char* d_out = c->di_out.as<unsigned char>();
    int64_t* d_meta = c->di_meta.as<int64_t>();
    HIP_TRY(c, hipMemcpyAsync(c->di_blob.p, blob, (size_t)n_blob, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_meta, lo, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_meta + n, hi, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_meta + 2 * n, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_out, 0xA5, (size_t)total + 2 * kGuard, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->di_status.p, 0, (size_t)(n + 2) * 4, c->stream));
    dinf_launch(c, c->di_blob.as<unsigned char>(), d_meta, n, d_out + kGuard, c->di_status.as<uint32_t>(), c->stream);
    HIP_TRY(c, hipGetLastError());
    unsigned char edge[2 * kGuard];
    HIP_TRY(c, hipMemcpyAsync(edge, d_out, kGuard, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(edge + kGuard, d_out + kGuard + total, kGuard, hipMemcpyDeviceToHost, c->stream));
    if (total) HIP_TRY(c, hipMemcpyAsync(out, d_out + kGuard, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, c->di_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    uint32_t any = 0;
    HIP_TRY(c, hipMemcpyAsync(&any, c->di_status.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < 2 * kGuard; ++i)
        if (edge[i] != 0xA5) return fail(c, WK_E_STATE, "the inflate kernel wrote outside the text (guard byte %zu)", i);
    bool failed = false;
    for (int64_t i = 0; i < n; ++i) failed = failed || status[i] != 0;
    if (failed != (any != 0)) return fail(c, WK_E_STATE, "the inflate kernel's failure word (%u) does not match its status words", any);
    return WK_OK;
}

// (measurement) text[begin, stop) to the device, to stay: a later wk_dtok_scan / wk_dtok_scan_emit of the same
// bytes finds them there and copies nothing.
int wk_text_upload(wk_ctx* c, const char* text, int64_t begin, int64_t stop) {
    if (!c || !text || begin < 0 || stop <= begin || stop - begin >= (1ll << 31) - 64) return WK_E_ARG;
    DeviceGuard guard(c->device);
    const uint32_t n = (uint32_t)(stop - begin);
    const uint32_t n_tiles = (n + kDtokTile - 1) / kDtokTile;
    wk_ctx::ResidentText r{};
    r.host = text + begin;
    r.n = n;
    void *dev = nullptr, *tiles = nullptr, *off = nullptr;
    HIP_TRY(c, hipMalloc(&dev, (size_t)n + 64));
    HIP_TRY(c, hipMalloc(&tiles, (size_t)n_tiles * 8));
    HIP_TRY(c, hipMalloc(&off, (size_t)n_tiles * 8));
    HIP_TRY(c, hipMemcpyAsync(dev, r.host, n, hipMemcpyHostToDevice, c->stream));
    // (the pad behind the text: dtok_count_kernel's last tile; the total: tile_scan_kernel stores it)
    count_newlines((const unsigned char*)dev, n, (unsigned long long*)tiles, (unsigned long long*)off, scalar_u64(c, 3), c->stream);
    HIP_TRY(c, hipMemcpyAsync(&r.n_newlines, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    (void)hipFree(tiles);
    r.dev = (unsigned char*)dev;
    r.tile_off = (unsigned long long*)off;
    c->resident.push_back(r);
    return WK_OK;
}

// (measurement) the rate of pinned host -> device copies of `bytes` each on this box, the way the text
// route makes them (hipMemcpyAsync from pinned memory on a stream of their own): bytes per second over
// `reps` copies back to back, timed with events.
int wk_h2d_rate(wk_ctx* c, int64_t bytes, int reps, double* bytes_per_s) {
    if (!c || bytes <= 0 || reps <= 0 || !bytes_per_s) return WK_E_ARG;
    DeviceGuard guard(c->device);
    void *h[2] = {nullptr, nullptr}, *d[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        for (int i = 0; i < 2; ++i) {
            if (h[i]) (void)hipHostFree(h[i]);
            if (d[i]) (void)hipFree(d[i]);
        }
        if (st) (void)hipStreamDestroy(st);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipHostMalloc(&h[i], (size_t)bytes, hipHostMallocDefault);
        if (e == hipSuccess) std::memset(h[i], 0x41 + i, (size_t)bytes);
        if (e == hipSuccess) e = hipMalloc(&d[i], (size_t)bytes);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMemcpyAsync(d[i], h[i], (size_t)bytes, hipMemcpyHostToDevice, st);  // warm
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int i = 0; i < reps && e == hipSuccess; ++i) e = hipMemcpyAsync(d[i & 1], h[i & 1], (size_t)bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    cleanup();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, WK_E_HIP, "wk_h2d_rate: %s", hipGetErrorString(e));
    }
    *bytes_per_s = ms > 0.f ? (double)bytes * reps / (ms * 1e-3) : 0.0;
    return WK_OK;
}

int wk_ordinal_chunk_counts(wk_ctx* c, int64_t* sorted, int64_t* gathered) {
    if (!c || !sorted || !gathered) return WK_E_ARG;
    *sorted = c->chunks_sorted;
    *gathered = c->chunks_gathered;
    return WK_OK;
}

// (measurement) blocks of the text route the fused kernel did / handed back to the six kernels since the context exists
int wk_dtok_fused_counts(wk_ctx* c, int64_t* done, int64_t* handed_back) {
    if (!c || !done || !handed_back) return WK_E_ARG;
    *done = c->fused_blocks;
    *handed_back = c->fused_fallbacks;
    return WK_OK;
}

// (measurement) The stamps the measuring instance of the one-kernel tokenizer left at its last launch with bit 4096 of
// "fz_ablate" (wk_dtok_fused.hpp, kFzTl*): the buffer is made here where no such launch has made it, the context's
// stream is waited for, and up to `cap` words go to `out`.
int wk_dtok_fused_timeline(wk_ctx* c, uint64_t* out, int64_t cap, int64_t* n_wgs, int64_t* words_per_wg, int64_t* every) {
    if (!c || !n_wgs || !words_per_wg || !every || cap < 0 || (cap > 0 && !out)) return WK_E_ARG;
    DeviceGuard guard(c->device);
    if (!c->d_timeline.p) {
        HIP_TRY(c, c->d_timeline.reserve((size_t)16 * kFzTlWords * 8));
        HIP_TRY(c, hipMemsetAsync(c->d_timeline.p, 0, c->d_timeline.cap, c->stream));
    }
    *n_wgs = c->tl_wgs;
    *words_per_wg = kFzTlWords;
    *every = kFzTlEvery;
    const int64_t have = (int64_t)c->tl_wgs * (int64_t)kFzTlWords, take = std::min(have, cap);
    if (take > 0) HIP_TRY(c, hipMemcpyAsync(out, c->d_timeline.p, (size_t)take * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

int wk_text_clear(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    for (wk_ctx::ResidentText& r : c->resident) {
        (void)hipFree(r.dev);
        (void)hipFree(r.tile_off);
    }
    c->resident.clear();
    return WK_OK;
}

// The tokenizer's ids are not the subject indices of the records (wk_set_subjects): map[id] is (`--trim-sub`, where
// several names are one subject).  n = 0: they are again.  Applies to the plain flavour's blocks from the next
// wk_dtok_emit / wk_dtok_scan_emit on; a block that meets an id beyond the map is the host tokenizer's.
int wk_dtok_subject_map(wk_ctx* c, const int32_t* map, int32_t n) {
    if (!c || n < 0 || (n > 0 && !map)) return WK_E_ARG;
    DeviceGuard guard(c->device);
    c->dt_submap_on = map != nullptr;  // (an empty map that is there: no name has been met yet)
    if (map && n == 0) HIP_TRY(c, c->d_submap.reserve(64));
    bool excl = false;
    if (n > 0) {
        for (int32_t i = 0; i < n; ++i) {
            if (map[i] == kLineExcluded)
                excl = true;
            else if (map[i] < 0)
                return fail(c, WK_E_ARG, "a subject map holds subject indices (or -4: excluded)");
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a kernel may be reading the map that is there)
        const int rc = upload(c, c->d_submap, map, (size_t)n * 4);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->dt_submap_n = (uint32_t)n;
    c->dt_has_excl = excl;
    return WK_OK;
}

int wk_dtok_format(wk_ctx* c, int fmt) {
    if (!c) return WK_E_ARG;
    if (fmt != WK_FMT_SAM && fmt != WK_FMT_MAP && fmt != WK_FMT_B6O && fmt != WK_FMT_PAF)
        return fail(c, WK_E_ARG, "the device tokenizer takes SAM, simple maps, BLAST tabular text and PAF");
    c->dt_fmt = fmt;
    return WK_OK;
}

static DevBuf& fz_bk(wk_ctx* c, int i) { return i == 0 ? c->w_backup : i == 1 ? c->w_backup2 : c->w_backup3; }

// The one-kernel tokenizer's geometry for a block of n bytes: one contiguous span per persistent workgroup
// ("dtok_fused_per_cu" of them per CU), the block in equal shares -- every workgroup walks the same number of bytes, and
// the halos in front of and behind a span are looked at once per workgroup, not once per 16 KB.  (64 MB over 768
// workgroups: spans of 85.3 KB, five windows each.)  Returns the grid; a short block gets fewer, 4 KB spans.
static unsigned fused_spans(const wk_ctx* c, uint32_t n, uint32_t* span) {
    const uint64_t wgs = (uint64_t)c->prop.multiProcessorCount * (uint64_t)c->fused_per_cu;
    const uint64_t share = (((uint64_t)n + wgs - 1) / wgs + 15u) & ~(uint64_t)15u;
    *span = (uint32_t)std::max<uint64_t>(share, 4096u);
    return (unsigned)(((uint64_t)n + *span - 1) / *span);
}

static int dtok_emit_launch(wk_ctx* c, bool* ordered_out, unsigned long long* totals);
static int dtok_emit_finish(wk_ctx* c, bool keep, bool ordered, DtokState st, unsigned long long totals, int64_t* n_reads,
                            int64_t* n_records);

// (measurement) The block as wk_text_upload left it on the device; null: it is not resident.
static const wk_ctx::ResidentText* resident_text(const wk_ctx* c, const char* src, uint32_t n) {
    const wk_ctx::ResidentText* res = nullptr;
    for (const wk_ctx::ResidentText& r : c->resident)
        if (r.host == src && r.n == n) res = &r;
    return res;
}

// The block's scalars and its list of subjects the dictionary does not hold.
static hipError_t dtok_scratch_reserve(wk_ctx* c) {
    const hipError_t e = c->d_state.reserve(sizeof(DtokState) + 64);
    return e != hipSuccess ? e : c->d_unknown.reserve((size_t)(1 << 20) * 8);
}

// (wk_dtok_expect) The records that the open sample's text will make, told from the lines per byte of the block
// scanned last, its first: a record per line at most; 8 % on top of the block's rate, never more than the 2^30 a pass
// holds.  words_room sizes the sample's record buffers from it.
static void words_expect_from_block(wk_ctx* c) {
    if (c->dt_expect_bytes <= 0 || c->w_expect != 0 || c->dt_n == 0) return;
    const double lines = (double)c->dt_expect_bytes * ((double)c->dt_lines / (double)c->dt_n) * 1.08 + (double)c->dt_lines;
    c->w_expect = (int64_t)std::min(lines, (double)(1ll << 30));
}

// ---- the one-kernel tokenizer (wk_dtok_fused.hpp) -----------------------------------------------------------------
// The usual block of a sample whose words are open -- SAM text, records for the weighted histogram, every subject
// known -- goes through ONE kernel.  A block it hands back (a subject the dictionary does not hold, a line for the
// host tokenizer, a run or a line beyond its window) leaves the streams as they were and takes the six kernels.
// This is what wk_dtok_scan_emit and wk_dtok_scan_emit_begin both ask of a block before they try the kernel; each adds
// its own: the flavour and `fz_skip`, which only the former counts down, there, the blocks under way here.
static bool fused_eligible(const wk_ctx* c, const wk_tok* tok) {
    return c->use_fused && c->dt_fmt == WK_FMT_SAM && c->w_open && c->w_mode == 0 && !c->dt_keep_reads &&
           wkx_tok_n_names(tok) < (1 << 23) - 1;
}

// Queue the kernel for the block of n bytes at `text`, its records to `streams` (at most kFzStreams of them).
// ONE launch per block while blocks follow one another through this kernel: its last workgroup leaves the cursors as
// they are behind the block in the next of three buffers -- the next block's "before" --, the block's scalars in
// pinned memory and cleared ones on the device.  fz_bk(ring) is this block's "before"; anything else that has moved
// the cursors or the scalars since the last launch has broken the chain (`fz_chain`): the small kernel in front, then.
// The scalars land in slot `host_slot` of the pinned scratch and, with seq != 0, that number 128 bytes into the slot
// once they are there.  Every field of FusedArgs is set here and nowhere else.
static int fused_launch(wk_ctx* c, const StreamSet& streams, const unsigned char* text, uint32_t n, bool open_end, int ring, int host_slot,
                        uint32_t seq) {
    static_assert(sizeof(DtokState) <= 128 && wk_ctx::kBackBytes >= 132, "the slot's second half holds the block's sequence number");
    FusedArgs fa{};
    const unsigned grid = fused_spans(c, n, &fa.span);
    if (fa.span % 16u) return fail(c, WK_E_ARG, "spans of the one-kernel tokenizer are multiples of 16 bytes");
    HIP_TRY(c, dtok_scratch_reserve(c));
    for (int i = 0; i < 3; ++i) HIP_TRY(c, fz_bk(c, i).reserve(kMaxStreams * 8));
    fa.text = text;
    fa.n = n;
    fa.open_end = open_end ? 1u : 0u;
    fa.dict8 = c->d_dict2.as<DictSlot8>();
    fa.names16 = c->d_names16.as<uint4>();
    fa.dict_mask = c->dt_dict_mask;
    fa.arena = c->d_arena.as<unsigned char>();
    fa.unknown = c->d_unknown.as<uint2>();
    fa.unknown_cap = (uint32_t)(c->d_unknown.cap / 8);
    fa.state = c->d_state.as<DtokState>();
    unsigned char* slot = c->host_back + (size_t)host_slot * wk_ctx::kBackBytes;
    fa.host_state = reinterpret_cast<DtokState*>(slot);
    fa.backup_prev = fz_bk(c, ring).as<unsigned long long>();   // (the block's records: the cursors' advance over it)
    fa.backup_next = fz_bk(c, (ring + 1) % 3).as<unsigned long long>();
    fa.host_seq = seq ? reinterpret_cast<uint32_t*>(slot + 128) : nullptr;
    fa.seq = seq;
    fa.streams = streams;
    fa.submap = c->dt_submap_on ? c->d_submap.as<int32_t>() : nullptr;
    fa.n_submap = c->dt_submap_n;
    fa.ablate = c->fused_ablate;
    fa.timeline = nullptr;  // (the product's instance never reads it)
    if (c->fused_ablate & kFzAblateTimeline) {  // (measurement: the buffer cleared in front of every launch that stamps)
        const uint32_t wgs = (grid + kFzTlEvery - 1u) / kFzTlEvery;
        HIP_TRY(c, c->d_timeline.reserve((size_t)std::max(wgs, 16u) * kFzTlWords * 8));
        HIP_TRY(c, hipMemsetAsync(c->d_timeline.p, 0, (size_t)wgs * kFzTlWords * 8, c->stream));
        fa.timeline = c->d_timeline.as<unsigned long long>();
        c->tl_wgs = wgs;
    }
    c->w_counts_known = false;
    KernelTimer* kf = ktimer_begin(c, "dtok_fused");
    if (!c->fz_chain)
        hipLaunchKernelGGL(dtok_fused_begin_kernel, dim3(1), dim3(64), 0, c->stream, fz_bk(c, ring).as<unsigned long long>(),
                           (const unsigned long long*)streams.cursor, fa.state);
    // (the measuring instance exactly when a phase is to be left out: the product's kernel holds no switch)
    if (c->fused_ablate != 0u)
        hipLaunchKernelGGL(dtok_fused_measure_kernel, dim3(grid), dim3(kFzThreads), 0, c->stream, fa);
    else
        hipLaunchKernelGGL(dtok_fused_kernel, dim3(grid), dim3(kFzThreads), 0, c->stream, fa);
    ktimer_end(c, kf);
    HIP_TRY(c, hipGetLastError());
    return WK_OK;
}

// The kernel kept a block of n bytes (`st`: its scalars; its records have been accepted).  Returns the block's lines.
static uint32_t fz_kept(wk_ctx* c, const DtokState& st, uint32_t n, bool open_end) {
    const uint32_t lines = (uint32_t)st.n_lines + (open_end ? 1u : 0u);
    c->dt_lines = lines;
    c->dt_lpb = (double)lines / (double)n;
    c->fused_streak = true;
    c->fz_back_streak = 0;
    ++c->fused_blocks;
    return lines;
}

// The kernel handed a block back (the cursors have been put back: the next launch seeds its "before" again).
static void fz_handed_back(wk_ctx* c) {
    c->fused_streak = false;
    c->fz_chain = false;
    ++c->fused_fallbacks;
    // (text the one kernel keeps handing back -- runs longer than its window, say -- pays for both ways block after
    // block: after two blocks in a row it is left out for 2, 4, ... 32 blocks before it is tried again)
    c->fz_back_streak = std::min(c->fz_back_streak + 1, 6);
    if (c->fz_back_streak >= 2) c->fz_skip = 1 << (c->fz_back_streak - 1);
}

// ---- wk_dtok_scan / wk_dtok_scan_emit: one block, step by step ------------------------------------------------
// The block on its way through dtok_scan_impl.
struct ScanBlock {
    wk_tok* tok;
    const char* src;        // the host's bytes: the block's tag, and its text unless c->dt_detached
    uint32_t n;
    bool extra;             // the "ex" flavour
    int64_t* n_lines;       // the caller's
    int* status;
    int* emit;
    int64_t* emitted;
    // where the text was found (the device pointer is c->dt_text)
    enum { kResident, kCopiedAhead, kCopiedNow } where;
    const wk_ctx::ResidentText* res;   // kResident
    int k;                             // otherwise: the text buffer
    bool counted;           // kCopiedAhead: the newlines were counted behind the copy
    bool open_end;          // a last line without newline
    bool fuse;              // the block tries the one kernel
    bool have_count;        // n_newlines and tile_off are there
    unsigned long long n_newlines;
    const unsigned long long* tile_off;
    uint32_t lines;         // counted, or (!have_count) what the block has at most
    KernelTimer* kt;        // the open bracket of family "dtok_lines"
    std::chrono::steady_clock::time_point lap_t;
};

static void scan_lap(wk_ctx* c, ScanBlock& s, int i) {
    const auto now = std::chrono::steady_clock::now();
    c->lap_x[i] += std::chrono::duration<double>(now - s.lap_t).count();
    s.lap_t = now;
}

// The block's records have been appended: what wk_dtok_scan_emit tells its caller then.
static void scan_reply_emitted(wk_ctx* c, const ScanBlock& s, int64_t n_reads, int64_t n_records) {
    *s.status = 0;
    *s.n_lines = s.lines;
    *s.emit = 1;
    s.emitted[0] = n_reads;
    s.emitted[1] = n_records;
    c->dt_ready = false;  // (nothing left for wk_dtok_emit)
}

// A block that has not been counted has no more lines than bytes / 7 -- a mapped record is "q\tf\tr\t\n" at least --
// and, once the sample has shown its lines per byte, a quarter more than that; the kernel reports records that find
// no room.
static uint32_t lines_at_most(const wk_ctx* c, uint32_t n) {
    double est = (double)n / 7.0 + 1.0;
    if (c->dt_lpb > 0.0) est = std::min(est, (double)n * c->dt_lpb * 1.25 + 65536.0);
    return (uint32_t)est;
}

// Is the block the device's at all?  (false: *status stays 1, the host tokenizer takes it)
static bool scan_checks(wk_ctx* c, ScanBlock& s, int64_t n64) {
    *s.status = 1;
    *s.n_lines = 0;
    c->dt_ready = false;
    c->dt_extra = s.extra;
    c->cv_line_next = 0;
    c->dx_looked = false;
    c->dx_runs = false;
    // (an exclusion set: the plain flavour takes it as kLineExcluded entries of the subject map, wk_dtok_subject_map;
    // the "ex" parsers' way with it -- align.py:481-547 yields a stale pool at the end of a file -- stays the host's)
    if (!wkx_tok_device_ok(s.tok) && (s.extra || !c->dt_submap_on)) return false;
    if (s.extra && c->dt_fmt == WK_FMT_MAP) return false;  // (a simple map has no "ex" flavour, align.py:236)
    if (n64 >= (1ll << 31) - 64) return false;
    s.n = (uint32_t)n64;
    return true;
}

// The block's text: resident (measurement), copied ahead by wk_dtok_copy (then the kernels only wait for that copy),
// or copied now.
static int scan_locate_text(wk_ctx* c, ScanBlock& s) {
    s.res = resident_text(c, s.src, s.n);
    s.where = ScanBlock::kResident;
    s.k = -1;
    s.lap_t = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lock(c->copy_mu);
        textbuf_release_scanned(c);
        c->dt_detached = false;
        if (!s.res && (s.k = textbuf_find_copied(c, s.src, s.n)) >= 0) {
            s.where = ScanBlock::kCopiedAhead;
            s.counted = c->text_buf[s.k].counted;
            c->dt_detached = c->text_buf[s.k].detached;
            textbuf_claim(c, s.k, wk_ctx::kBufScanning);   // (the buffer's tag is used up)
        } else if (!s.res) {
            s.where = ScanBlock::kCopiedNow;
            if ((s.k = textbuf_take_free(c, wk_ctx::kBufScanning)) < 0) return fail(c, WK_E_STATE, "every text buffer holds a block copied ahead");
        }
    }
    if (s.where == ScanBlock::kResident) {
        c->dt_text = s.res->dev;   // (64 zero bytes behind it)
    } else {
        TextBuf& b = c->text_buf[s.k];
        if (s.where == ScanBlock::kCopiedAhead) {
            HIP_TRY(c, hipStreamWaitEvent(c->stream, b.ev, 0));  // (the pad: zeroed by the count behind the copy)
        } else {
            HIP_TRY(c, text_buffer(c, s.k, (size_t)s.n + 64));
            HIP_TRY(c, copy_text_async(c, b.text, s.src, s.n, c->stream));  // (the pad: zeroed by the count below)
        }
        c->dt_text = b.text;
    }
    scan_lap(c, s, 0);
    return WK_OK;
}

// The block's newlines per tile and their offsets into d_tiles / d_tile_off, the total into scalar 3, on the scan's
// stream; `wait`: and the stream waited for, the count taken.
static int scan_count_now(wk_ctx* c, ScanBlock& s, bool wait) {
    const uint32_t n_tiles = (s.n + kDtokTile - 1) / kDtokTile;
    HIP_TRY(c, c->d_tiles.reserve((size_t)n_tiles * 8));
    HIP_TRY(c, c->d_tile_off.reserve((size_t)n_tiles * 8));
    count_newlines(c->dt_text, s.n, c->d_tiles.as<unsigned long long>(), c->d_tile_off.as<unsigned long long>(), scalar_u64(c, 3), c->stream);
    if (!wait) return WK_OK;
    HIP_TRY(c, hipMemcpyAsync(&s.n_newlines, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    s.tile_off = c->d_tile_off.as<unsigned long long>();
    s.have_count = true;
    return WK_OK;
}

// Which way does the block go, and how many lines has it?  The six kernels need the block's newlines per tile before
// anything else; the one kernel counts its lines itself.  A block copied ahead while blocks went through the one
// kernel (`fused_streak`) was not counted behind its copy: it is counted here only if it needs the six kernels -- it
// may still turn out to (scan_line_starts) -- or if the sample's record buffers are still to be sized from its lines
// per byte (wk_dtok_expect).
static int scan_count(wk_ctx* c, ScanBlock& s) {
    HIP_TRY(c, dtok_scratch_reserve(c));
    s.fuse = s.emit && !s.extra && fused_eligible(c, s.tok);
    if (s.fuse && c->fz_skip > 0) {   // (left out after blocks handed back in a row: fz_handed_back)
        --c->fz_skip;
        s.fuse = false;
    }
    s.kt = ktimer_begin(c, "dtok_lines");
    if (s.where == ScanBlock::kResident) {
        // (the product counts a block's newlines behind its copy -- when the block is to take the six kernels -- and
        // never waits for them; here the same two kernels run in front of the scan, their result was taken at upload)
        int rc = 0;
        if (!s.fuse && (rc = scan_count_now(c, s, false))) return rc;
        s.n_newlines = s.res->n_newlines;
        s.tile_off = s.res->tile_off;
        s.have_count = true;
    } else if (s.counted) {  // (counted behind the copy: the number is on the host once the copy's event has passed)
        const TextBuf& b = c->text_buf[s.k];
        {
            Lap wait(&c->lap_s[3]);
            HIP_TRY(c, hipEventSynchronize(b.ev));
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, b.ev0, b.evm) == hipSuccess) {
            c->lap_copy_ms += ms;
            c->lap_copy_bytes += s.n;
        } else {
            (void)hipGetLastError();
        }
        s.n_newlines = c->copy_newlines[s.k];
        s.tile_off = b.tile_off.as<unsigned long long>();
        s.have_count = true;
    } else if (!s.fuse || (c->dt_expect_bytes > 0 && c->w_expect == 0)) {
        const int rc = scan_count_now(c, s, true);
        if (rc) return rc;
    }
    // (the last byte was noted when the block was copied ahead: the host bytes of such a block may be gone)
    s.open_end = (s.where == ScanBlock::kCopiedAhead ? c->text_buf[s.k].last : s.src[s.n - 1]) != '\n';
    s.lines = s.have_count ? (uint32_t)s.n_newlines + (s.open_end ? 1u : 0u) : lines_at_most(c, s.n);
    return WK_OK;
}

// The one kernel, waited for at once; *done: it kept the block and the caller has its answer.  Its scalars land in
// slot 0 of the pinned scratch.  `fz_parity` moves on only when the block is kept.
static int scan_try_fused(wk_ctx* c, ScanBlock& s, bool* done) {
    c->dt_lines = s.lines;
    int rc = dtok_mirror_dict(c, s.tok);
    if (rc) return rc;
    words_expect_from_block(c);   // (the block has been counted then: scan_count)
    if ((rc = words_roll(c, s.lines))) return rc;
    if ((rc = words_room(c, s.lines))) return rc;
    // (words_roll may have reopened the job set: the block takes the six kernels then and counts as no hand-back)
    const StreamSet streams = stream_set(c);
    if (c->w_mode != 0 || streams.n_streams > kFzStreams) return WK_OK;
    if (s.where == ScanBlock::kResident) ktimer_end(c, s.kt);   // (the count behind a resident block's "copy": its own family)
    const int ring = c->fz_parity;
    if ((rc = fused_launch(c, streams, c->dt_text, s.n, s.open_end, ring, 0, 0))) return rc;
    c->w_backup_cur = fz_bk(c, ring).p;
    scan_lap(c, s, 2);
    DtokState st{};
    {
        Lap wait(&c->lap_s[2]);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    small_back_get(c, 0, &st, sizeof st);
    s.lap_t = std::chrono::steady_clock::now();
    const bool keep = st.flags == 0 && st.n_unknown == 0;
    int64_t nr = 0, nrec = 0;
    c->dt_emitted = false;
    if ((rc = dtok_emit_finish(c, keep, false, st, 0, &nr, &nrec))) return rc;   // (not kept: the cursors go back)
    scan_lap(c, s, 4);
    if (!keep) {
        fz_handed_back(c);
        s.kt = ktimer_begin(c, "dtok_lines");
        return WK_OK;
    }
    c->fz_chain = true;
    c->fz_parity = (ring + 1) % 3;
    s.lines = fz_kept(c, st, s.n, s.open_end);
    scan_reply_emitted(c, s, nr, nrec);
    *done = true;
    return WK_OK;
}

// Line starts (the first of the six kernels): offsets per tile -> positions.
static int scan_line_starts(wk_ctx* c, ScanBlock& s) {
    if (!s.have_count) {  // (the six kernels after all)
        const int rc = scan_count_now(c, s, true);
        if (rc) return rc;
        s.lines = (uint32_t)s.n_newlines + (s.open_end ? 1u : 0u);
    }
    c->fused_streak = false;
    // (sized for a full block of short lines from the first block on: a file's first blocks are small, and
    // every growth is a hipFree -- which waits for the device -- and a hipMalloc per array)
    const size_t cap_lines = std::max<size_t>(s.lines, (size_t)1 << 21);
    HIP_TRY(c, c->d_lines.reserve((cap_lines + 2) * 4));
    HIP_TRY(c, c->d_lsubj.reserve((cap_lines + 1) * 4));
    HIP_TRY(c, c->d_lmeta.reserve((cap_lines + 1) * 4));
    HIP_TRY(c, c->d_start.reserve(cap_lines + 64));
    HIP_TRY(c, c->d_first.reserve(cap_lines + 64));
    if (s.extra) {
        HIP_TRY(c, c->d_lbeg.reserve((cap_lines + 1) * 4));
        HIP_TRY(c, c->d_lend.reserve((cap_lines + 1) * 4));
        HIP_TRY(c, c->d_llen.reserve((cap_lines + 1) * 4));
        HIP_TRY(c, c->d_lscan.reserve((cap_lines + 1) * 8));
    }
    // (line 0 and the block's scalars are written by the lines kernel itself)
    hipLaunchKernelGGL(dtok_lines_kernel, dim3((s.n + kDtokTile - 1) / kDtokTile), dim3(kDtokThreads), 0, c->stream, c->dt_text, s.n,
                       s.tile_off, c->d_lines.as<uint32_t>(), c->d_state.as<DtokState>());
    if (s.open_end) {
        const uint32_t end = s.n + 1;  // as if a newline followed the text
        HIP_TRY(c, hipMemcpyAsync(c->d_lines.as<uint32_t>() + s.lines, &end, 4, hipMemcpyHostToDevice, c->stream));
    }
    ktimer_end(c, s.kt);
    HIP_TRY(c, hipGetLastError());
    c->dt_lines = s.lines;
    scan_lap(c, s, 1);
    return WK_OK;
}

// The subjects that the parse did not find in the dictionary (d_unknown: offset and length of each name) are
// interned, in text order -- from the host's bytes, or from the device's where those are gone.
static int scan_intern_unknown(wk_ctx* c, const ScanBlock& s, uint32_t n_unknown) {
    std::vector<uint2> unk(n_unknown);
    HIP_TRY(c, hipMemcpyAsync(unk.data(), c->d_unknown.p, (size_t)n_unknown * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::sort(unk.begin(), unk.end(), [](const uint2& x, const uint2& y) { return x.x < y.x; });
    if (!c->dt_detached) {
        for (const uint2& u : unk) (void)wkx_tok_intern(s.tok, s.src + u.x, u.y);
        return WK_OK;
    }
    // the names come back from the device: one by one while they are few, with the whole block otherwise
    const bool whole = unk.size() > 128;
    size_t need = 0;
    for (const uint2& u : unk) need += u.y;
    std::vector<char> back(whole ? (size_t)s.n : need);
    if (whole) {
        HIP_TRY(c, hipMemcpyAsync(back.data(), c->dt_text, s.n, hipMemcpyDeviceToHost, c->stream));
    } else {
        size_t at = 0;
        for (const uint2& u : unk) {
            if (u.y) HIP_TRY(c, hipMemcpyAsync(back.data() + at, c->dt_text + u.x, u.y, hipMemcpyDeviceToHost, c->stream));
            at += u.y;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    size_t at = 0;
    for (const uint2& u : unk) {
        (void)wkx_tok_intern(s.tok, back.data() + (whole ? (size_t)u.x : at), u.y);
        at += u.y;
    }
    return WK_OK;
}

// Parse (with the emission queued right behind it where the caller takes one); subjects the dictionary does not know
// are interned, then once more.
static int scan_parse_rounds(wk_ctx* c, ScanBlock& s) {
    for (int round = 0; round < 3; ++round) {
        int rc = dtok_mirror_dict(c, s.tok);
        if (rc) return rc;
        if (round > 0) HIP_TRY(c, hipMemsetAsync(c->d_state.p, 0, sizeof(DtokState), c->stream));  // (round 0: by dtok_lines_kernel)
        const DtokArgs a = dtok_args(c);
        c->dt_mapped = false;
        const dim3 grid((s.lines + kDtokThreads - 1) / kDtokThreads);
        KernelTimer* kt = ktimer_begin(c, "dtok_parse");
        if (s.extra)
            hipLaunchKernelGGL(dtok_parse_kernel<true>, grid, dim3(kDtokThreads), 0, c->stream, a);
        else
            hipLaunchKernelGGL(dtok_parse_kernel<false>, grid, dim3(kDtokThreads), 0, c->stream, a);
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        scan_lap(c, s, 2);
        const bool speculate = s.emit && round == 0 && !s.extra && c->w_open && s.lines > 0;
        bool ordered = false;
        unsigned long long totals = 0;
        if (speculate && (rc = dtok_emit_launch(c, &ordered, &totals))) return rc;
        scan_lap(c, s, 3);
        DtokState st{};
        static_assert(sizeof(DtokState) <= (size_t)wk_ctx::kBackBytes && sizeof(DtokState) % 4 == 0, "DtokState fits a slot");
        HIP_TRY(c, small_back(c, 0, c->d_state.p, sizeof st));
        {
            Lap wait(&c->lap_s[2]);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        small_back_get(c, 0, &st, sizeof st);
        if (speculate && ordered) small_back_get(c, 1, &totals, 8);
        s.lap_t = std::chrono::steady_clock::now();
        if (speculate) {
            const bool keep = st.flags == 0 && st.n_unknown == 0;
            int64_t nr = 0, nrec = 0;
            if ((rc = dtok_emit_finish(c, keep, ordered, st, totals, &nr, &nrec))) return rc;
            scan_lap(c, s, 4);
            if (keep) {
                scan_reply_emitted(c, s, nr, nrec);
                return WK_OK;
            }
        }
        if (st.flags) return WK_OK;  // status 1: the host tokenizer takes the block
        if (st.n_unknown == 0) {
            *s.status = 0;
            *s.n_lines = s.lines;
            c->dt_ready = true;
            return WK_OK;
        }
        s.lap_t = std::chrono::steady_clock::now();
        if ((rc = scan_intern_unknown(c, s, (uint32_t)st.n_unknown))) return rc;
        scan_lap(c, s, 5);
    }
    return fail(c, WK_E_STATE, "device tokenizer: subjects still unknown after interning them");
}

// `emit` (may be null): with the words of this sample open (wk_words_begin), the emission is queued right behind the
// parse — the usual block brings no subject the dictionary does not know — and the host waits once for both; *emit = 1
// when the block's records have been appended that way (then emitted[0..1] = reads, records).
static int dtok_scan_impl(wk_ctx* c, wk_tok* tok, const char* text, int64_t begin, int64_t stop, int extra, int64_t* n_lines, int* status,
                          int* emit, int64_t* emitted) {
    if (!c || !tok || !text || begin < 0 || stop < begin || !n_lines || !status) return WK_E_ARG;
    if (emit) *emit = 0;
    if (c->lag_count) return fail(c, WK_E_STATE, "blocks whose verdict has not been read (wk_dtok_scan_emit_end)");
    Lap lap(&c->lap_s[1]);
    ScanBlock s{tok, text + begin, 0, extra != 0, n_lines, status, emit, emitted};
    if (!scan_checks(c, s, stop - begin)) return WK_OK;
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    c->dt_n = s.n;
    c->dt_lines = 0;
    if (s.n == 0) {
        *status = 0;
        c->dt_ready = true;
        return WK_OK;
    }
    int rc;
    if ((rc = scan_locate_text(c, s))) return rc;
    if ((rc = scan_count(c, s))) return rc;
    if (s.fuse) {
        bool done = false;
        if ((rc = scan_try_fused(c, s, &done)) || done) return rc;
    }
    if ((rc = scan_line_starts(c, s))) return rc;
    return scan_parse_rounds(c, s);
}

// ---- the verdict of a block read one block late ------------------------------------------------------------------
// wk_dtok_scan_emit waits for a block's kernel before the next block's is launched: the device idles while the host
// wakes up, reads the verdict and launches again (14 of a block's 138 us with the text resident).  _begin launches a
// block's one-kernel tokenizer and returns; _end waits for the OLDEST block launched that way and says what became of
// it.  With two blocks under way the second one's kernel starts the moment the first one's ends.  A block the kernel
// hands back (*status = 2) has left no record -- nor has the block launched behind it, which is forgotten: the caller
// scans both again the synchronous way (their text is where it was).
// (The launch is made as if the block will be kept: `fz_parity` moves on and `fz_chain` is set at once, `w_backup_cur`
// is _end's to set when it keeps the block.  A hand-back does not rewind the parity: the broken chain seeds the next
// launch's "before" again.)
int wk_dtok_scan_emit_begin(wk_ctx* c, wk_tok* tok, const char* text, int64_t begin, int64_t stop, int* started) {
    if (!c || !tok || !text || begin < 0 || stop < begin || !started) return WK_E_ARG;
    *started = 0;
    const int64_t n64 = stop - begin;
    if (!c->lag_enabled || c->lag_count >= 2 || c->fz_skip > 0 || n64 <= 0 || n64 >= (1ll << 31) - 64 || !fused_eligible(c, tok)) return WK_OK;
    if (!wkx_tok_device_ok(tok) && !c->dt_submap_on) return WK_OK;
    if (c->dt_expect_bytes > 0 && c->w_expect == 0) return WK_OK;   // (the sample's buffers are sized from a counted block)
    if (c->lag_count > 0 && !c->fz_chain) return WK_OK;
    DeviceGuard guard(c->device);
    const uint32_t n = (uint32_t)n64;
    const char* src = text + begin;
    const wk_ctx::ResidentText* res = resident_text(c, src, n);
    int k = -1;
    {
        std::lock_guard<std::mutex> lock(c->copy_mu);
        if (c->lag_count == 0) textbuf_release_scanned(c);
        if (!res && (k = textbuf_find_copied(c, src, n)) < 0) return WK_OK;   // (not copied ahead: the synchronous call copies it)
    }
    uint32_t lines = 0;
    bool open_end;
    if (res) {
        open_end = src[n - 1] != '\n';
        lines = (uint32_t)res->n_newlines + (open_end ? 1u : 0u);
    } else {
        if (c->dt_lpb <= 0.0) return WK_OK;
        open_end = c->text_buf[k].last != '\n';
        lines = lines_at_most(c, n);
    }
    // room for the records of every block under way (none of them is in w_records yet); a buffer that would have to
    // grow while a kernel appends to it, or a sample that would have to be rolled, waits for the verdicts
    int64_t under_way = lines;
    for (int i = 0; i < c->lag_count; ++i) under_way += c->lag[i].lines_est;
    if (c->w_records + under_way >= (1ll << 30) - (1 << 20)) return WK_OK;
    if (c->w_sliced && streams_needed(c) > kMaxStreams) return WK_OK;
    if (c->lag_count == 0) {
        const int rcw = words_room(c, under_way);
        if (rcw) return rcw;
    } else {
        const int want = c->w_sliced ? streams_needed(c) : 1;
        const size_t need = (size_t)(c->w_records + under_way) * 4 + 64;
        bool fits = c->w_cursor.p != nullptr && c->w_streams >= want;
        for (int q = 0; fits && q < c->w_streams; ++q) fits = need <= c->w_stream[q].cap;
        if (!fits) return WK_OK;
    }
    int rc = dtok_mirror_dict(c, tok);
    if (rc) return rc;
    const StreamSet streams = stream_set(c);
    if (streams.n_streams > kFzStreams) return WK_OK;
    if (!res) {
        {
            std::lock_guard<std::mutex> lock(c->copy_mu);
            textbuf_claim(c, k, wk_ctx::kBufPending);
        }
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->text_buf[k].ev, 0));
    }
    wk_ctx::LagSlot& L = c->lag[c->lag_count];
    L.buf = k;
    L.src = src;
    L.n = n;
    L.open_end = open_end;
    L.ring = c->fz_parity;
    L.lines_est = lines;
    L.host_slot = 2 + c->lag_next_ev;
    if (!c->lag_ev[c->lag_next_ev]) HIP_TRY(c, hipEventCreateWithFlags(&c->lag_ev[c->lag_next_ev], hipEventDisableTiming));
    L.ev = c->lag_ev[c->lag_next_ev];
    c->lag_next_ev ^= 1;
    L.seq = 0;   // (the block's end is seen in pinned memory; without `lag_poll`, waited for through L.ev)
    if (c->lag_poll) L.seq = ++c->lag_seq ? c->lag_seq : ++c->lag_seq;
    KtScope kt_scope(c);   // (wk_profile_kernels: a block queued behind another one is bracketed from that one's end to its own)
    if ((rc = fused_launch(c, streams, res ? res->dev : c->text_buf[k].text, n, open_end, L.ring, L.host_slot, L.seq))) return rc;
    if (!c->lag_poll) HIP_TRY(c, hipEventRecord(L.ev, c->stream));
    // (the next block is launched as if this one will be kept: its kernel leaves what that needs behind)
    c->fz_chain = true;
    c->fz_parity = (c->fz_parity + 1) % 3;
    ++c->lag_count;
    *started = 1;
    return WK_OK;
}

// *status: 0 = the oldest block under way has been appended (*n_reads, *n_records, *n_lines), 2 = the kernel handed it
// back: no block under way has left a record, none is under way any more, and the synchronous calls find their text.
int wk_dtok_scan_emit_end(wk_ctx* c, int64_t* n_lines, int* status, int64_t* n_reads, int64_t* n_records) {
    if (!c || !n_lines || !status || !n_reads || !n_records) return WK_E_ARG;
    if (c->lag_count == 0) return fail(c, WK_E_STATE, "no block under way (wk_dtok_scan_emit_begin)");
    DeviceGuard guard(c->device);
    const wk_ctx::LagSlot L = c->lag[0];
    if (L.seq) {
        // (the kernel's last workgroup stores the number behind the block's scalars: looked for every few
        // microseconds -- there is a whole kernel's time of slack --, the stream waited for if it does not show)
        const volatile uint32_t* seen = reinterpret_cast<const volatile uint32_t*>(c->host_back + (size_t)L.host_slot * wk_ctx::kBackBytes + 128);
        const auto t0 = std::chrono::steady_clock::now();
        bool there = false;
        for (int spin = 0;; ++spin) {
            if (__atomic_load_n(const_cast<const uint32_t*>(reinterpret_cast<const volatile uint32_t*>(seen)), __ATOMIC_ACQUIRE) == L.seq) {
                there = true;
                break;
            }
            if (spin < 64) continue;
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.01) break;
            struct timespec ts = {0, 5000};
            nanosleep(&ts, nullptr);
        }
        if (!there) HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
        HIP_TRY(c, hipEventSynchronize(L.ev));
    }
    DtokState st{};
    small_back_get(c, L.host_slot, &st, sizeof st);
    const bool keep = st.flags == 0 && st.n_unknown == 0;
    *n_lines = *n_reads = *n_records = 0;
    if (keep) {
        c->w_backup_cur = fz_bk(c, L.ring).p;
        c->dt_emitted = false;
        const int rc = dtok_emit_finish(c, true, false, st, 0, n_reads, n_records);
        if (rc) return rc;
        *n_lines = fz_kept(c, st, L.n, L.open_end);
        *status = 0;
        if (L.buf >= 0) {
            std::lock_guard<std::mutex> lock(c->copy_mu);
            c->text_buf[L.buf].state = wk_ctx::kBufFree;
        }
        c->lag[0] = c->lag[1];
        --c->lag_count;
        return WK_OK;
    }
    // handed back: every kernel under way through, the cursors as they were in front of this block -- which takes the
    // records of the block behind it along --, the blocks' text findable again
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->w_cursor.p, fz_bk(c, L.ring).p, kMaxStreams * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    {
        std::lock_guard<std::mutex> lock(c->copy_mu);
        for (int i = 0; i < c->lag_count; ++i)
            if (c->lag[i].buf >= 0) textbuf_retag(c, c->lag[i].buf, c->lag[i].src, c->lag[i].n);
    }
    c->lag_count = 0;
    fz_handed_back(c);
    *status = 2;
    return WK_OK;
}

int wk_dtok_scan(wk_ctx* c, wk_tok* tok, const char* text, int64_t begin, int64_t stop, int extra, int64_t* n_lines, int* status) {
    return dtok_scan_impl(c, tok, text, begin, stop, extra, n_lines, status, nullptr, nullptr);
}

int wk_dtok_scan_emit(wk_ctx* c, wk_tok* tok, const char* text, int64_t begin, int64_t stop, int64_t* n_lines, int* status, int* emitted,
                      int64_t* n_reads, int64_t* n_records) {
    if (!emitted || !n_reads || !n_records) return WK_E_ARG;
    int64_t out[2] = {0, 0};
    const int rc = dtok_scan_impl(c, tok, text, begin, stop, 0, n_lines, status, emitted, out);
    *n_reads = out[0];
    *n_records = out[1];
    return rc;
}

// The emission of a scanned block in two halves, so that wk_dtok_scan_emit can queue it behind the parse without
// waiting in between: `launch` queues the kernels (and, where the records are placed by prefix sums, the copy of their
// totals), `finish` — once the stream has been waited for — accepts or discards what they wrote.
static int dtok_emit_launch(wk_ctx* c, bool* ordered_out, unsigned long long* totals) {
    c->fz_chain = false;
    words_expect_from_block(c);
    int rc = words_roll(c, c->dt_lines);
    if (rc) return rc;
    if ((rc = words_room(c, c->dt_lines))) return rc;
    DtokArgs a = dtok_args(c);
    if (c->w_mode == 0) {
        a.streams = stream_set(c);
        c->w_counts_known = false;
        // (a block the kernels give up on must leave the streams as they were)
        HIP_TRY(c, c->w_backup.reserve(kMaxStreams * 8));
        a.cursor_backup = c->w_backup.as<unsigned long long>();  // (copied by dtok_runs_kernel)
        c->w_backup_cur = c->w_backup.p;
    } else {
        a.out = c->c_words.as<uint32_t>() + c->w_records;
        a.out_cap = c->dt_lines;
    }
    const dim3 grid((c->dt_lines + kDtokThreads - 1) / kDtokThreads);
    const dim3 emit_grid((c->dt_lines + kDtokThreads * kScatterItems - 1) / (kDtokThreads * kScatterItems));
    KernelTimer* kt = ktimer_begin(c, "dtok_emit");
    hipLaunchKernelGGL(dtok_runs_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
    if (a.submap && !c->dt_mapped) {  // (once per scanned block; behind the runs: a line of an excluded subject starts and continues runs like any other)
        hipLaunchKernelGGL(dtok_submap_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
        if (c->dt_has_excl) {
            HIP_TRY(c, hipMemsetAsync(c->d_first.p, 0, c->dt_lines, c->stream));
            hipLaunchKernelGGL(dtok_excl_mark_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
            hipLaunchKernelGGL(dtok_excl_drop_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
        }
        c->dt_mapped = true;
    }
    const bool ordered = c->w_mode != 0 || c->dt_keep_reads;
    *ordered_out = ordered;
    c->dt_emitted = false;
    if (ordered) hipLaunchKernelGGL(dtok_first_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
    if (ordered) {
        // the per-read stream wants the records of a read next to each other, in
        // position order: placed by prefix sums instead of appended wave by wave
        const uint32_t n_tiles = grid.x;
        HIP_TRY(c, c->d_tiles.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, c->d_tile_off.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, c->d_lscan.reserve(((size_t)c->dt_lines + 1) * 8));
        a.line_scan = c->d_lscan.as<unsigned long long>();
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
        hipLaunchKernelGGL(dtok_hits_kernel<false>, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tiles.as<unsigned long long>());
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                           c->d_tile_off.as<unsigned long long>(), (int64_t)n_tiles, scalar_u64(c, 3));
        hipLaunchKernelGGL(dtok_scan_lines_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tile_off.as<unsigned long long>());
        if (c->w_mode == 0)  // (read maps wanted, records for the histogram: by slice, in no particular order)
            hipLaunchKernelGGL(dtok_emit_kernel, emit_grid, dim3(kDtokThreads), 0, c->stream, a);
        else
            hipLaunchKernelGGL(dtok_place_words_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
        (void)totals;  // (slot 1 of the pinned scratch: read by the caller once the stream has been waited for)
        HIP_TRY(c, small_back(c, 1, scalar_u64(c, 3), 8));
    } else {
        // (first-line flags and emission in one kernel, the runs' lines staged in LDS)
        hipLaunchKernelGGL(dtok_first_emit_kernel, emit_grid, dim3(kDtokThreads), 0, c->stream, a);
    }
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    return WK_OK;
}

// (the stream has been waited for) `keep` false: the streams' cursors go back to where they were
static int dtok_emit_finish(wk_ctx* c, bool keep, bool ordered, DtokState st, unsigned long long totals, int64_t* n_reads,
                            int64_t* n_records) {
    if (ordered) {
        st.n_out = totals & 0xFFFFFFFFull;
        st.n_reads = totals >> 32;
    }
    if (!keep) {
        if (c->w_mode == 0) {
            c->fz_chain = false;
            HIP_TRY(c, hipMemcpyAsync(c->w_cursor.p, c->w_backup_cur, kMaxStreams * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        return WK_OK;
    }
    c->dt_emitted = c->dt_keep_reads;
    c->dt_emit_reads = (uint32_t)st.n_reads;
    const int rc = words_translate(c, c->w_records, (int64_t)st.n_out);
    if (rc) return rc;
    c->w_records += (int64_t)st.n_out;
    c->w_reads += (int64_t)st.n_reads;
    *n_reads = (int64_t)st.n_reads;
    *n_records = (int64_t)st.n_out;
    return WK_OK;
}

int wk_dtok_emit(wk_ctx* c, int64_t* n_reads, int64_t* n_records, int* status) {
    if (!c || !n_reads || !n_records || !status) return WK_E_ARG;
    *status = 1;
    *n_reads = *n_records = 0;
    // (an "ex" block while a coverage pile is open: its ranges went to the pile, wk_dtok_cover_append; its lines' subjects,
    // query lengths and mates are what the plain parse leaves, so the records come from the same kernels)
    if (!c->dt_ready || (c->dt_extra && !c->cv_open)) return fail(c, WK_E_STATE, "no block scanned for the plain flavour (wk_dtok_scan)");
    if (!c->w_open) return fail(c, WK_E_STATE, "wk_words_begin has not accepted a job set");
    c->dt_ready = false;
    if (c->dt_lines == 0) {
        *status = 0;
        return WK_OK;
    }
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    bool ordered = false;
    unsigned long long totals = 0;
    int rc = dtok_emit_launch(c, &ordered, &totals);
    if (rc) return rc;
    DtokState st{};
    HIP_TRY(c, small_back(c, 0, c->d_state.p, sizeof st));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    small_back_get(c, 0, &st, sizeof st);
    if (ordered) small_back_get(c, 1, &totals, 8);
    // (a read of more than 16 subjects: nothing counts as appended)
    if ((rc = dtok_emit_finish(c, st.flags == 0, ordered, st, totals, n_reads, n_records))) return rc;
    if (st.flags == 0) *status = 0;
    return WK_OK;
}

// ---- subject coverage on the device (wk_cover.hpp) ------------------------------------------------------------------

// the pile's scalars (after everything queued so far)
static int cover_read_state(wk_ctx* c) {
    static_assert(sizeof(CoverState) <= (size_t)wk_ctx::kBackBytes && sizeof(CoverState) % 4 == 0, "CoverState fits a slot");
    HIP_TRY(c, small_back(c, 1, c->cv_state.p, sizeof(CoverState)));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    small_back_get(c, 1, &c->cv_seen, sizeof(CoverState));
    if (c->cv_seen.overflow || c->cv_seen.tail > (unsigned long long)c->cv_cap)
        return fail(c, WK_E_STATE, "coverage pile: rows beyond the room reserved for them");
    c->cv_tail = c->cv_ub = (int64_t)c->cv_seen.tail;
    c->cv_stale = false;
    return WK_OK;
}

// The exact tail is wanted when room runs out, not behind every append: until then cv_ub (every line handed over counted
// as a row) stands in for it, and a block's ranges cost no wait of their own.
static int cover_sync(wk_ctx* c) { return c->cv_stale ? cover_read_state(c) : WK_OK; }

static int cover_clear(wk_ctx* c) {
    CoverState st{};
    st.key_and = ~0ull;
    st.end_and = ~0u;
    HIP_TRY(c, hipMemcpyAsync(c->cv_state.p, &st, sizeof st, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->cv_seen = st;
    c->cv_tail = c->cv_merged = c->cv_ub = 0;
    c->cv_stale = false;
    c->cv_cur = 0;
    return WK_OK;
}

// Sort the pile and merge it: the merged set is the pile afterwards (in the other buffer of the sorted rows).
static int cover_compact(wk_ctx* c) {
    int rc = cover_sync(c);
    if (rc) return rc;
    if (c->cv_tail == c->cv_merged) return WK_OK;  // (nothing behind the merged set)
    const uint32_t n = (uint32_t)c->cv_tail;
    KernelTimer* kt = ktimer_begin(c, "cover_sort");
    // the digits that differ between rows: of `end` first when rows with end < beg are about (a sort by (subject, beg,
    // end) then, as merge_ranges'), then of the key
    const uint32_t n_chunks = (n + kCoverChunk - 1) / kCoverChunk;
    const uint32_t n_matrix = 256u * n_chunks;
    const uint32_t n_mtiles = (n_matrix + kCoverTile - 1) / kCoverTile;
    int cur = c->cv_cur;
    auto pass = [&](uint32_t from_end, uint32_t shift) {
        CoverSortArgs a{};
        a.key_in = c->cv_key[cur].as<unsigned long long>();
        a.end_in = c->cv_end[cur].as<int32_t>();
        a.key_out = c->cv_key[cur ^ 1].as<unsigned long long>();
        a.end_out = c->cv_end[cur ^ 1].as<int32_t>();
        a.n = n;
        a.n_chunks = n_chunks;
        a.shift = shift;
        a.from_end = from_end;
        a.hist = c->cv_hist.as<uint32_t>();
        a.st = c->cv_state.as<CoverState>();
        const dim3 grid((n_chunks + kCoverWaves - 1) / kCoverWaves);
        hipLaunchKernelGGL(cover_hist_kernel, grid, dim3(kCoverThreads), 0, c->stream, a);
        hipLaunchKernelGGL(cover_sum_tiles_kernel, dim3(n_mtiles), dim3(kCoverThreads), 0, c->stream, (const uint32_t*)a.hist, n_matrix,
                           c->cv_tiles.as<unsigned long long>());
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->cv_tiles.as<unsigned long long>(),
                           c->cv_tile_off.as<unsigned long long>(), (int64_t)n_mtiles, scalar_u64(c, 3));
        hipLaunchKernelGGL(cover_scan_apply_kernel, dim3(n_mtiles), dim3(kCoverThreads), 0, c->stream, a.hist, n_matrix,
                           (const unsigned long long*)c->cv_tile_off.as<unsigned long long>());
        hipLaunchKernelGGL(cover_scatter_kernel, grid, dim3(kCoverThreads), 0, c->stream, a);
        cur ^= 1;
    };
    const uint32_t end_diff = c->cv_seen.end_or ^ c->cv_seen.end_and;
    const unsigned long long key_diff = c->cv_seen.key_or ^ c->cv_seen.key_and;
    if (c->cv_seen.degenerate)
        for (uint32_t b = 0; b < 4; ++b)
            if ((end_diff >> (8 * b)) & 255u) pass(1, 8 * b);
    for (uint32_t b = 0; b < 8; ++b)
        if ((key_diff >> (8 * b)) & 255ull) pass(0, 8 * b);
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    kt = ktimer_begin(c, "cover_merge");
    const uint32_t n_tiles = (n + kCoverTile - 1) / kCoverTile;
    CoverMergeArgs m{};
    m.key = c->cv_key[cur].as<unsigned long long>();
    m.end = c->cv_end[cur].as<int32_t>();
    m.n = n;
    m.reach = c->cv_reach.as<int32_t>();
    m.tile_max = c->cv_tiles.as<unsigned long long>();
    m.tile_heads = c->cv_tiles.as<unsigned long long>() + n_tiles;
    m.tile_off = c->cv_tile_off.as<unsigned long long>();
    m.key_out = c->cv_key[cur ^ 1].as<unsigned long long>();
    m.end_out = c->cv_end[cur ^ 1].as<int32_t>();
    hipLaunchKernelGGL(cover_max_tiles_kernel, dim3(n_tiles), dim3(kCoverThreads), 0, c->stream, m);
    hipLaunchKernelGGL(cover_max_scan_kernel, dim3(1), dim3(1024), 0, c->stream, m.tile_max, n_tiles);
    hipLaunchKernelGGL(cover_reach_kernel, dim3(n_tiles), dim3(kCoverThreads), 0, c->stream, m);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, m.tile_heads, c->cv_tile_off.as<unsigned long long>(),
                       (int64_t)n_tiles, scalar_u64(c, 3));
    hipLaunchKernelGGL(cover_compact_kernel, dim3(n_tiles), dim3(kCoverThreads), 0, c->stream, m);
    hipLaunchKernelGGL(cover_set_tail_kernel, dim3(1), dim3(1), 0, c->stream, c->cv_state.as<CoverState>(),
                       (const unsigned long long*)scalar_u64(c, 3));
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    c->cv_cur = cur ^ 1;
    if ((rc = cover_read_state(c))) return rc;
    if (c->cv_tail > (int64_t)n) return fail(c, WK_E_STATE, "coverage pile: more merged ranges than rows");
    c->cv_merged = c->cv_tail;
    return WK_OK;
}

// Room for up to `want` more rows: how many of them may be appended now (0: the merged set alone fills more than half the
// pile -- the caller fetches it, resets and comes back).  Compacts when the tail has no room for them.
static int cover_room(wk_ctx* c, int64_t want, int64_t* room) {
    *room = c->cv_cap - c->cv_ub;
    if (*room >= want) return WK_OK;
    int rc = cover_sync(c);  // (the bound says no: the exact tail may say yes)
    if (rc) return rc;
    *room = c->cv_cap - c->cv_tail;
    if (*room >= want) return WK_OK;
    if (*room < c->cv_cap / 4) {
        if ((rc = cover_compact(c))) return rc;
        *room = c->cv_merged > c->cv_cap / 2 ? 0 : c->cv_cap - c->cv_tail;
    }
    return WK_OK;
}

static void cover_append_launch(wk_ctx* c, const int32_t* subj, const int32_t* beg, const int32_t* end, uint32_t i0, uint32_t i1) {
    hipLaunchKernelGGL(cover_append_kernel, dim3((i1 - i0 + kCoverThreads - 1) / kCoverThreads), dim3(kCoverThreads), 0, c->stream, subj, beg, end,
                       i0, i1, c->cv_key[c->cv_cur].as<unsigned long long>(), c->cv_end[c->cv_cur].as<int32_t>(), (unsigned long long)c->cv_cap,
                       c->cv_state.as<CoverState>());
}

int wk_cover_begin(wk_ctx* c, int64_t cap_rows) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    if (cap_rows < 0) {  // the pile is given up
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (DevBuf* b : {&c->cv_key[0], &c->cv_key[1], &c->cv_end[0], &c->cv_end[1], &c->cv_reach, &c->cv_hist, &c->cv_tiles, &c->cv_tile_off,
                          &c->cv_stage[0], &c->cv_stage[1], &c->cv_stage[2]})
            b->release();
        c->cv_open = false;
        c->cv_cap = c->cv_tail = c->cv_merged = c->cv_ub = 0;
        c->cv_stale = false;
        return WK_OK;
    }
    if (cap_rows == 0) cap_rows = c->cv_cap_opt ? c->cv_cap_opt : kCoverCapDefault;
    if (cap_rows < kCoverCapMin || cap_rows > kCoverCapMax)
        return fail(c, WK_E_ARG, "a coverage pile holds %lld to %lld rows", (long long)kCoverCapMin, (long long)kCoverCapMax);
    // (the merge's threads load whole tiles: the buffers end at a tile's end)
    const size_t rows = ((size_t)cap_rows + kCoverTile - 1) / kCoverTile * kCoverTile;
    const size_t n_chunks = ((size_t)cap_rows + kCoverChunk - 1) / kCoverChunk;
    const size_t n_mtiles = (256 * n_chunks + kCoverTile - 1) / kCoverTile;
    const size_t n_tiles = rows / kCoverTile;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c, c->cv_key[k].reserve(rows * 8));
        HIP_TRY(c, c->cv_end[k].reserve(rows * 4));
    }
    HIP_TRY(c, c->cv_reach.reserve(rows * 4));
    HIP_TRY(c, c->cv_hist.reserve(256 * n_chunks * 4));
    HIP_TRY(c, c->cv_tiles.reserve(std::max(n_mtiles, 2 * n_tiles) * 8));
    HIP_TRY(c, c->cv_tile_off.reserve(std::max(n_mtiles, n_tiles) * 8));
    HIP_TRY(c, c->cv_state.reserve(sizeof(CoverState)));
    c->cv_cap = cap_rows;
    c->cv_open = true;
    return cover_clear(c);
}

int wk_cover_reset(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    if (!c->cv_open) return fail(c, WK_E_STATE, "no coverage pile (wk_cover_begin)");
    DeviceGuard guard(c->device);
    return cover_clear(c);
}

int wk_cover_add(wk_ctx* c, const int32_t* subj, const int32_t* beg, const int32_t* end, int64_t n, int64_t* n_taken) {
    if (!c || n < 0 || !n_taken || (n > 0 && (!subj || !beg || !end))) return WK_E_ARG;
    *n_taken = 0;
    if (!c->cv_open) return fail(c, WK_E_STATE, "no coverage pile (wk_cover_begin)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    while (*n_taken < n) {
        int64_t room = 0;
        int rc = cover_room(c, n - *n_taken, &room);
        if (rc) return rc;
        if (room == 0) return WK_OK;  // (*n_taken < n: the pile is full of merged ranges)
        const int64_t take = std::min(room, n - *n_taken);
        const int32_t* src[3] = {subj + *n_taken, beg + *n_taken, end + *n_taken};
        for (int k = 0; k < 3; ++k)
            if ((rc = upload(c, c->cv_stage[k], src[k], (size_t)take * 4))) return rc;
        KernelTimer* kt = ktimer_begin(c, "cover_append");
        cover_append_launch(c, c->cv_stage[0].as<int32_t>(), c->cv_stage[1].as<int32_t>(), c->cv_stage[2].as<int32_t>(), 0u, (uint32_t)take);
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        // (the staged rows are read by the kernel: waited for before the next piece overwrites them)
        if ((rc = cover_read_state(c))) return rc;
        *n_taken += take;
    }
    return WK_OK;
}

// The ranges of the block scanned last ("ex" flavour) -> the pile: every line with a subject (the tokenizer's id: coverage
// is keyed by the name in the file).  *full = 1: the pile is full of merged ranges and lines of the block are left --
// after wk_cover_fetch + wk_cover_reset the same call goes on where it stopped.
int wk_dtok_cover_append(wk_ctx* c, int64_t* n_lines, int* full) {
    if (!c || !n_lines || !full) return WK_E_ARG;
    *n_lines = 0;
    *full = 0;
    if (!c->cv_open) return fail(c, WK_E_STATE, "no coverage pile (wk_cover_begin)");
    if (!c->dt_ready || !c->dt_extra) return fail(c, WK_E_STATE, "no block scanned for the \"ex\" flavour (wk_dtok_scan)");
    if (c->dt_mapped) return fail(c, WK_E_STATE, "the block's subjects have been translated already (wk_dtok_emit)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    while (c->cv_line_next < c->dt_lines) {
        const int64_t left = (int64_t)c->dt_lines - c->cv_line_next;
        int64_t room = 0;
        int rc = cover_room(c, left, &room);
        if (rc) return rc;
        if (room == 0) {
            *full = 1;
            break;
        }
        const uint32_t take = (uint32_t)std::min(room, left);
        KernelTimer* kt = ktimer_begin(c, "cover_append");
        cover_append_launch(c, c->d_lsubj.as<int32_t>(), c->d_lbeg.as<int32_t>(), c->d_lend.as<int32_t>(), c->cv_line_next, c->cv_line_next + take);
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        c->cv_ub += take;
        c->cv_stale = true;
        c->cv_line_next += take;
        *n_lines += take;
    }
    return WK_OK;
}

int wk_cover_finish(wk_ctx* c, int64_t* n_ranges) {
    if (!c || !n_ranges) return WK_E_ARG;
    *n_ranges = 0;
    if (!c->cv_open) return fail(c, WK_E_STATE, "no coverage pile (wk_cover_begin)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    const int rc = cover_compact(c);
    if (rc) return rc;
    *n_ranges = c->cv_merged;
    return WK_OK;
}

int wk_cover_fetch(wk_ctx* c, int32_t* subj, int32_t* beg, int32_t* end, int64_t cap) {
    if (!c || cap < 0 || (cap > 0 && (!subj || !beg || !end))) return WK_E_ARG;
    if (!c->cv_open) return fail(c, WK_E_STATE, "no coverage pile (wk_cover_begin)");
    if (c->cv_stale || c->cv_tail != c->cv_merged) return fail(c, WK_E_STATE, "rows behind the merged set (wk_cover_finish)");
    const int64_t n = c->cv_merged;
    if (n > cap) return fail(c, WK_E_CAPACITY, "need room for %lld merged ranges", (long long)n);
    if (n == 0) return WK_OK;
    DeviceGuard guard(c->device);
    std::vector<unsigned long long> keys((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(keys.data(), c->cv_key[c->cv_cur].p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(end, c->cv_end[c->cv_cur].p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; ++i) {
        subj[i] = (int32_t)(keys[(size_t)i] >> 32);
        beg[i] = (int32_t)((uint32_t)keys[(size_t)i] ^ kCoverBias);
    }
    return WK_OK;
}

// ---- strata map on the device (wk_strata.hpp) ---------------------------------------

static StrataArgs strata_args(wk_ctx* c) {
    StrataArgs s{};
    s.text = c->s_text.as<unsigned char>();
    s.n = c->s_n;
    s.line_start = c->s_lines.as<uint32_t>();
    s.n_lines = c->s_n_lines;
    s.line_tab = c->s_tab.as<uint32_t>();
    s.line_vlen = c->s_vlen.as<uint32_t>();
    s.line_hash = c->s_hash.as<unsigned long long>();
    s.line_label = c->s_label.as<uint32_t>();
    s.slots = c->s_slots.as<StrataSlot>();
    s.mask = c->s_mask;
    s.labels = c->s_labels.as<LabelSlot>();
    s.label_text = c->s_label_text.as<uint2>();
    s.label_group = c->s_label_group.as<int32_t>();
    s.state = c->s_state.as<uint32_t>();
    return s;
}

int wk_strata_clear(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    c->s_ready = c->s_use = false;
    return WK_OK;
}

int wk_strata_load(wk_ctx* c, const char* text, int64_t n64, int64_t* n_pairs, int32_t* n_labels, int* status) {
    if (!c || n64 < 0 || (n64 > 0 && !text) || !n_pairs || !n_labels || !status) return WK_E_ARG;
    *status = 1;
    *n_pairs = 0;
    *n_labels = 0;
    c->s_ready = c->s_use = false;
    if (n64 >= (1ll << 32) - 64) return WK_OK;  // (offsets are 32 bits: the host's join takes larger maps)
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    const uint32_t n = (uint32_t)n64;
    c->s_n = n;
    c->s_n_lines = 0;
    HIP_TRY(c, c->s_state.reserve(64));
    HIP_TRY(c, hipMemsetAsync(c->s_state.p, 0, 64, c->stream));
    HIP_TRY(c, c->s_labels.reserve((size_t)kStrataLabelSlots * sizeof(LabelSlot)));
    HIP_TRY(c, c->s_label_text.reserve((size_t)kStrataLabelSlots * 8));
    HIP_TRY(c, c->s_label_group.reserve((size_t)kStrataLabelSlots * 4));
    HIP_TRY(c, hipMemsetAsync(c->s_labels.p, 0xFF, (size_t)kStrataLabelSlots * sizeof(LabelSlot), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->s_label_group.p, 0xFF, (size_t)kStrataLabelSlots * 4, c->stream));
    if (n == 0) {
        HIP_TRY(c, c->s_slots.reserve(1024 * sizeof(StrataSlot)));
        HIP_TRY(c, hipMemsetAsync(c->s_slots.p, 0, 1024 * sizeof(StrataSlot), c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->s_mask = 1023;
        c->s_ready = true;
        *status = 0;
        return WK_OK;
    }
    HIP_TRY(c, c->s_text.reserve((size_t)n + 64));
    HIP_TRY(c, copy_text_async(c, c->s_text.p, text, n, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->s_text.as<unsigned char>() + n, 0, 64, c->stream));
    // line starts, like a block of alignment text
    const uint32_t n_tiles = (n + kDtokTile - 1) / kDtokTile;
    HIP_TRY(c, c->s_tiles.reserve((size_t)n_tiles * 8));
    HIP_TRY(c, c->s_tile_off.reserve((size_t)n_tiles * 8));
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
    count_newlines(c->s_text.as<unsigned char>(), n, c->s_tiles.as<unsigned long long>(), c->s_tile_off.as<unsigned long long>(),
                   scalar_u64(c, 3), c->stream);
    unsigned long long n_newlines = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_newlines, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const bool open_end = text[n - 1] != '\n';
    const uint32_t lines = (uint32_t)n_newlines + (open_end ? 1u : 0u);
    HIP_TRY(c, c->s_lines.reserve(((size_t)lines + 2) * 4));
    HIP_TRY(c, c->s_tab.reserve(((size_t)lines + 1) * 4));
    HIP_TRY(c, c->s_vlen.reserve(((size_t)lines + 1) * 4));
    HIP_TRY(c, c->s_hash.reserve(((size_t)lines + 1) * 8));
    HIP_TRY(c, c->s_label.reserve(((size_t)lines + 1) * 4));
    uint64_t slots = 1024;
    while (slots < 2ull * lines) slots <<= 1;
    HIP_TRY(c, c->s_slots.reserve((size_t)slots * sizeof(StrataSlot)));
    HIP_TRY(c, hipMemsetAsync(c->s_slots.p, 0, (size_t)slots * sizeof(StrataSlot), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->s_lines.p, 0, 4, c->stream));
    hipLaunchKernelGGL(dtok_lines_kernel, dim3(n_tiles), dim3(kDtokThreads), 0, c->stream, c->s_text.as<unsigned char>(), n,
                       c->s_tile_off.as<unsigned long long>(), c->s_lines.as<uint32_t>());
    if (open_end) {
        const uint32_t end = n + 1;
        HIP_TRY(c, hipMemcpyAsync(c->s_lines.as<uint32_t>() + lines, &end, 4, hipMemcpyHostToDevice, c->stream));
    }
    c->s_n_lines = lines;
    c->s_mask = (uint32_t)(slots - 1);
    const StrataArgs s = strata_args(c);
    const dim3 grid((lines + kStrataThreads - 1) / kStrataThreads);
    KernelTimer* kt = ktimer_begin(c, "strata");
    hipLaunchKernelGGL(strata_parse_kernel, grid, dim3(kStrataThreads), 0, c->stream, s);
    hipLaunchKernelGGL(strata_verify_kernel, grid, dim3(kStrataThreads), 0, c->stream, s);
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    uint32_t st[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(st, c->s_state.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st[0]) return WK_OK;  // status 1: the host's join takes the sample
    c->s_ready = true;
    *n_pairs = st[1];
    *n_labels = (int32_t)st[2];
    *status = 0;
    return WK_OK;
}

int wk_strata_labels(wk_ctx* c, int32_t* slot, int64_t* text_off, int32_t* text_len, int32_t cap, int32_t* n_out) {
    if (!c || !n_out || cap < 0 || (cap > 0 && (!slot || !text_off || !text_len))) return WK_E_ARG;
    *n_out = 0;
    if (!c->s_ready) return fail(c, WK_E_STATE, "no strata map on the device (wk_strata_load)");
    DeviceGuard guard(c->device);
    std::vector<LabelSlot> tab(kStrataLabelSlots);
    std::vector<uint2> txt(kStrataLabelSlots);
    HIP_TRY(c, hipMemcpyAsync(tab.data(), c->s_labels.p, tab.size() * sizeof(LabelSlot), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(txt.data(), c->s_label_text.p, txt.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // in the order their first lines appear in the map
    std::vector<std::pair<uint32_t, uint32_t>> order;  // (first line, slot)
    for (uint32_t q = 0; q < kStrataLabelSlots; ++q)
        if (tab[q].hash != kLabelEmpty) order.emplace_back(tab[q].rep, q);
    std::sort(order.begin(), order.end());
    if ((int64_t)order.size() > cap) return fail(c, WK_E_CAPACITY, "need room for %zu labels", order.size());
    for (size_t k = 0; k < order.size(); ++k) {
        const uint32_t q = order[k].second;
        slot[k] = (int32_t)q;
        text_off[k] = txt[q].x;
        text_len[k] = (int32_t)txt[q].y;
    }
    *n_out = (int32_t)order.size();
    return WK_OK;
}

int wk_strata_groups(wk_ctx* c, const int32_t* slot, const int32_t* group, int32_t n) {
    if (!c || n < 0 || (n > 0 && (!slot || !group))) return WK_E_ARG;
    if (!c->s_ready) return fail(c, WK_E_STATE, "no strata map on the device (wk_strata_load)");
    std::vector<int32_t> all(kStrataLabelSlots, -1);
    for (int32_t k = 0; k < n; ++k) {
        if (slot[k] < 0 || (uint32_t)slot[k] >= kStrataLabelSlots) return fail(c, WK_E_ARG, "label slot outside the table");
        if (group[k] >= (1 << WK_KEY_GROUP_BITS)) return fail(c, WK_E_ARG, "group id outside [0, %d)", 1 << WK_KEY_GROUP_BITS);
        all[slot[k]] = group[k];
    }
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(c->s_label_group.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->s_use = true;
    return WK_OK;
}

// ---- read maps on the device (wk_readmap.hpp) -------------------------------------

int wk_dtok_keep_reads(wk_ctx* c, int on) {
    if (!c) return WK_E_ARG;
    c->dt_keep_reads = on != 0;
    if (!on) c->dt_emitted = false;
    return WK_OK;
}

int wk_readmap_tables(wk_ctx* c, int32_t job, const int32_t* slot_of_subject, int32_t n_subjects, const int32_t* slot_order,
                      const uint32_t* shown_off, const char* shown, int32_t n_slots) {
    if (!c) return WK_E_ARG;
    if (job < 0 || job >= WK_MAX_JOBS) return fail(c, WK_E_ARG, "job must be in [0, %d)", WK_MAX_JOBS);
    if (n_subjects < 0 || n_slots < 0 || (n_subjects > 0 && !slot_of_subject) || (n_slots > 0 && (!slot_order || !shown_off)))
        return fail(c, WK_E_ARG, "bad read-map tables");
    for (int32_t s = 0; s < n_subjects; ++s)
        if (slot_of_subject[s] < 0 || slot_of_subject[s] >= n_slots) return fail(c, WK_E_ARG, "subject %d has no taxon slot", s);
    DeviceGuard guard(c->device);
    wk_ctx::MapTables& T = c->rm[job];
    static const uint32_t zero = 0;
    int rc;
    if ((rc = upload(c, T.slot_of_subject, slot_of_subject, (size_t)n_subjects * 4))) return rc;
    if ((rc = upload(c, T.slot_order, slot_order, (size_t)n_slots * 4))) return rc;
    if ((rc = upload(c, T.shown_off, n_slots > 0 ? shown_off : &zero, ((size_t)n_slots + 1) * 4))) return rc;
    const size_t n_text = n_slots > 0 ? shown_off[n_slots] : 0;
    if (n_text > 0 && !shown) return fail(c, WK_E_ARG, "bad read-map tables");
    if ((rc = upload(c, T.shown, shown, n_text))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's buffers are only valid during the call)
    T.n_subjects = n_subjects;
    T.n_slots = n_slots;
    return WK_OK;
}

int wk_dtok_readmap(wk_ctx* c, int32_t job, int64_t* n_bytes) {
    if (!c || !n_bytes) return WK_E_ARG;
    *n_bytes = 0;
    c->rm_bytes = 0;
    if (job < 0 || job >= WK_MAX_JOBS) return fail(c, WK_E_ARG, "job must be in [0, %d)", WK_MAX_JOBS);
    if (!c->dt_emitted) return fail(c, WK_E_STATE, "no block emitted with its reads kept (wk_dtok_keep_reads, wk_dtok_emit)");
    const wk_ctx::MapTables& T = c->rm[job];
    if (T.n_subjects < c->n_subjects) return fail(c, WK_E_STATE, "read-map tables of job %d cover %d of %d subjects", job, T.n_subjects, c->n_subjects);
    const uint32_t n_reads = c->dt_emit_reads;
    if (n_reads == 0 || c->dt_lines == 0) return WK_OK;
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    HIP_TRY(c, c->rm_line.reserve((size_t)n_reads * 4));
    HIP_TRY(c, c->rm_len.reserve((size_t)n_reads * 8));
    DtokArgs a = dtok_args(c);
    ReadmapArgs m{};
    m.slot_of_subject = T.slot_of_subject.as<int32_t>();
    m.n_subjects = (uint32_t)T.n_subjects;
    m.slot_order = T.slot_order.as<int32_t>();
    m.shown_off = T.shown_off.as<uint32_t>();
    m.shown = T.shown.as<unsigned char>();
    m.read_line = c->rm_line.as<uint32_t>();
    m.read_len = c->rm_len.as<unsigned long long>();
    m.n_reads = n_reads;
    const dim3 lgrid((c->dt_lines + kDtokThreads - 1) / kDtokThreads), rgrid((n_reads + kDtokThreads - 1) / kDtokThreads);
    HIP_TRY(c, c->d_tiles.reserve((size_t)rgrid.x * 8));
    HIP_TRY(c, c->d_tile_off.reserve((size_t)rgrid.x * 8));
    HIP_TRY(c, hipMemsetAsync(c->rm_len.p, 0, (size_t)n_reads * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
    KernelTimer* kt = ktimer_begin(c, "readmap");
    hipLaunchKernelGGL(readmap_len_kernel, lgrid, dim3(kDtokThreads), 0, c->stream, a, m);
    hipLaunchKernelGGL(u64_tile_sum_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, m.read_len, n_reads, c->d_tiles.as<unsigned long long>());
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                       c->d_tile_off.as<unsigned long long>(), (int64_t)rgrid.x, scalar_u64(c, 3));
    hipLaunchKernelGGL(u64_tile_prefix_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, m.read_len, n_reads, c->d_tile_off.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (total >= (1ull << 40)) return fail(c, WK_E_RANGE, "read-map text of one block beyond 2^40 bytes");
    if (total > 0) {
        HIP_TRY(c, c->rm_text.reserve((size_t)total + 64));
        m.out = c->rm_text.as<unsigned char>();
        m.out_cap = total;
        hipLaunchKernelGGL(readmap_write_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, m);
        HIP_TRY(c, hipGetLastError());
    }
    ktimer_end(c, kt);
    c->rm_bytes = (int64_t)total;
    *n_bytes = (int64_t)total;
    return WK_OK;
}

int wk_dtok_readmap_fetch(wk_ctx* c, char* out, int64_t cap) {
    if (!c) return WK_E_ARG;
    if (c->rm_bytes == 0) return WK_OK;
    if (!out || cap < c->rm_bytes) return fail(c, WK_E_CAPACITY, "need %lld bytes", (long long)c->rm_bytes);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(out, c->rm_text.p, (size_t)c->rm_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// The scanned block's hits ("ex" flavour) as the staged chunk of the coord-match:
// what wk_ordinal_stage would have been given.  `append`: behind the hits staged by the calls before that
// nothing has counted yet (a read's hits never span two blocks: the chunk of both is what wk_ordinal_stage
// would have been given for their reads together).
static hipError_t grow_keep(wk_ctx* c, DevBuf& b, size_t need, size_t keep) {
    if (need <= b.cap) return hipSuccess;
    if (keep == 0 || !b.p) return b.reserve(need);
    DevBuf bigger;
    hipError_t e = bigger.reserve(need * 2);
    if (e != hipSuccess && (e = bigger.reserve(need)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(bigger.p, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice, c->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    b.release();
    b = bigger;
    return hipSuccess;
}

static int reads_runs_once(wk_ctx* c, const DtokArgs& a, dim3 grid);

static int dtok_stage_impl(wk_ctx* c, const int32_t* genome_of_subject, int32_t n_subjects, double th, bool append, int64_t* n_reads,
                           int64_t* n_hits, int* status) {
    if (!c || !n_reads || !n_hits || !status || n_subjects < 0 || (n_subjects > 0 && !genome_of_subject)) return WK_E_ARG;
    *status = 1;
    *n_reads = *n_hits = 0;
    if (!c->dt_ready || !c->dt_extra) return fail(c, WK_E_STATE, "no block scanned for the \"ex\" flavour (wk_dtok_scan)");
    if (!(th > 0.0)) return fail(c, WK_E_ARG, "overlap threshold must be positive");
    if (c->acc_open && !append) return fail(c, WK_E_STATE, "staged hits not counted yet (wk_ordinal_count)");
    if (c->acc_open && th != c->th) return fail(c, WK_E_STATE, "staged hits of another overlap threshold not counted yet");
    c->dt_ready = false;
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    const uint32_t lines = c->dt_lines;
    const bool behind = append && c->acc_open && c->ord_valid;
    const int64_t base_h = behind ? c->n_hits : 0, base_r = behind ? c->o_reads : 0;
    if (base_h + (int64_t)lines >= (1ll << 31) - 64) return fail(c, WK_E_RANGE, "more than 2^31 hits staged");
    int rc;
    if ((rc = upload(c, c->d_gmap, genome_of_subject, (size_t)std::max(n_subjects, 1) * 4))) return rc;
    const size_t cap_h = (size_t)base_h + lines + 1, keep_h = (size_t)base_h * 4;
    HIP_TRY(c, grow_keep(c, c->o_genome, cap_h * 4, keep_h));
    HIP_TRY(c, grow_keep(c, c->o_beg, cap_h * 4, keep_h));
    HIP_TRY(c, grow_keep(c, c->o_end, cap_h * 4, keep_h));
    HIP_TRY(c, grow_keep(c, c->o_len, cap_h * 4, keep_h));
    HIP_TRY(c, grow_keep(c, c->o_hoff, ((size_t)base_r + lines + 2) * 4, (size_t)base_r * 4));
    unsigned long long totals = 0;
    if (lines > 0) {
        DtokArgs a = dtok_args(c);
        a.gmap = c->d_gmap.as<int32_t>();
        a.n_gmap = (uint32_t)n_subjects;
        a.o_genome = c->o_genome.as<int32_t>() + base_h;
        a.o_beg = c->o_beg.as<int32_t>() + base_h;
        a.o_end = c->o_end.as<int32_t>() + base_h;
        a.o_len = c->o_len.as<uint32_t>() + base_h;
        a.o_hoff = c->o_hoff.as<int32_t>() + base_r;
        a.o_hit_base = (uint32_t)base_h;
        const uint32_t n_tiles = (lines + kDtokThreads - 1) / kDtokThreads;
        HIP_TRY(c, c->d_tiles.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, c->d_tile_off.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
        const dim3 grid(n_tiles);
        KernelTimer* kt = ktimer_begin(c, "dtok_emit");
        if ((rc = reads_runs_once(c, a, grid))) return rc;
        hipLaunchKernelGGL(dtok_hits_kernel<true>, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tiles.as<unsigned long long>());
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                           c->d_tile_off.as<unsigned long long>(), (int64_t)n_tiles, scalar_u64(c, 3));
        hipLaunchKernelGGL(dtok_scan_lines_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tile_off.as<unsigned long long>());
        if (c->s_use) {
            HIP_TRY(c, grow_keep(c, c->c_group, ((size_t)base_r + lines + 1) * 4, (size_t)base_r * 4));
            a.o_group = c->c_group.as<int32_t>() + base_r;
            hipLaunchKernelGGL(dtok_place_kernel<true>, grid, dim3(kDtokThreads), 0, c->stream, a, strata_args(c));
        } else {
            hipLaunchKernelGGL(dtok_place_kernel<false>, grid, dim3(kDtokThreads), 0, c->stream, a, StrataArgs{});
        }
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, small_back(c, 1, scalar_u64(c, 3), 8));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        small_back_get(c, 1, &totals, 8);
    }
    const int64_t hits = (int64_t)(totals & 0xFFFFFFFFull), reads = (int64_t)(totals >> 32);
    // (the offsets' last entry; the stream orders it in front of whatever reads them)
    hipLaunchKernelGGL(store_u32_kernel, dim3(1), dim3(1), 0, c->stream, c->o_hoff.as<uint32_t>() + base_r + reads, (uint32_t)(base_h + hits));
    HIP_TRY(c, hipGetLastError());
    c->n_hits = base_h + hits;
    c->o_reads = base_r + reads;
    c->th = th;
    c->has_group = c->s_use && (lines > 0 || (behind && c->has_group));
    c->group_base = 0;
    c->rk_valid[0] = c->rk_valid[1] = false;
    c->ord_valid = true;
    c->sb_valid = false;
    c->chunk_valid = false;
    c->acc_open = append;
    c->dx_chunk = false;
    c->rr_chunk = false;
    c->rd_chunk = false;
    c->dx_hits = false;
    *n_reads = reads;
    *n_hits = hits;
    *status = 0;
    return WK_OK;
}

int wk_dtok_stage_hits(wk_ctx* c, const int32_t* genome_of_subject, int32_t n_subjects, double th, int64_t* n_reads,
                       int64_t* n_hits, int* status) {
    return dtok_stage_impl(c, genome_of_subject, n_subjects, th, false, n_reads, n_hits, status);
}

// ---- demultiplexing on the device (wk_demux.hpp) ---------------------------------------------------------------------

static uint32_t demux_max(const wk_ctx* c) { return c->dx_max_opt ? (uint32_t)c->dx_max_opt : kDemuxMaxSamples; }

static DemuxArgs demux_args(wk_ctx* c) {
    DemuxArgs d{};
    d.tab = c->dx_tab.as<DemuxSlot>();
    d.name_off = c->dx_name_off.as<uint2>();
    d.arena = c->dx_arena.as<unsigned char>();
    d.group = c->dx_group.as<int32_t>();
    d.met = c->dx_met.as<unsigned char>();
    d.pend = c->dx_pend.as<DemuxPend>();
    d.pend_list = c->dx_pend_list.as<uint32_t>();
    d.state = c->dx_state.as<uint32_t>();
    d.lsamp = c->dx_lsamp.as<int32_t>();
    d.hash_mask = c->dx_hash_mask;
    const uint32_t known = (uint32_t)c->dx_name_off_host.size(), most = demux_max(c);
    d.max_new = most > known ? most - known : 0u;
    return d;
}

int wk_demux_begin(wk_ctx* c, int on) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->dx_on = on != 0;
    c->dx_looked = false;
    c->dx_chunk = false;
    c->rr_chunk = false;
    c->rd_chunk = false;
    c->dx_hits = false;
    c->dx_groups_n = 0;
    c->dx_name_off_host.clear();
    c->dx_arena_host.clear();
    c->dx_tab_host.assign(on ? kDemuxSlots : 0u, DemuxSlot{0ull, 0u, 0u});
    if (!on) return WK_OK;
    static_assert(sizeof(DemuxSlot) == 16 && sizeof(DemuxPend) == 16, "16-byte slots");
    HIP_TRY(c, c->dx_tab.reserve((size_t)kDemuxSlots * sizeof(DemuxSlot)));
    HIP_TRY(c, c->dx_pend.reserve((size_t)kDemuxSlots * sizeof(DemuxPend)));
    HIP_TRY(c, c->dx_pend_list.reserve((size_t)kDemuxMaxSamples * 4));
    HIP_TRY(c, c->dx_met.reserve(kDemuxMaxSamples));
    HIP_TRY(c, c->dx_name_off.reserve(64));
    HIP_TRY(c, c->dx_arena.reserve(64));
    HIP_TRY(c, c->dx_group.reserve(64));
    HIP_TRY(c, c->dx_state.reserve(64));
    HIP_TRY(c, hipMemsetAsync(c->dx_tab.p, 0, (size_t)kDemuxSlots * sizeof(DemuxSlot), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// run starts, subject map and exclusion set of the scanned block (as dtok_emit_launch has them), queued once per scanned
// block: the runs are told with every mapped line in place -- a run the exclusion set drops still separates its
// neighbours
static int reads_runs_once(wk_ctx* c, const DtokArgs& a, dim3 grid) {
    if (c->dx_runs) return WK_OK;
    hipLaunchKernelGGL(dtok_runs_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
    if (a.submap && !c->dt_mapped && !c->dt_extra) {  // (the "ex" flavour's ids go through `genome_of_subject`)
        hipLaunchKernelGGL(dtok_submap_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
        if (c->dt_has_excl) {
            HIP_TRY(c, hipMemsetAsync(c->d_first.p, 0, c->dt_lines, c->stream));
            hipLaunchKernelGGL(dtok_excl_mark_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
            hipLaunchKernelGGL(dtok_excl_drop_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
        }
        c->dt_mapped = true;
    }
    c->dx_runs = true;
    return WK_OK;
}

// run starts, subject map and exclusion set of the scanned block, then the lookup of its reads' samples; the pending
// names end up in dx_pend_*
static int demux_lookup(wk_ctx* c) {
    c->dx_pend_off.clear();
    c->dx_pend_len.clear();
    c->dx_pend_blob.clear();
    c->dx_status = 1;
    const uint32_t lines = c->dt_lines;
    if (lines == 0) {
        c->dx_status = 0;
        c->dx_looked = true;
        return WK_OK;
    }
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    HIP_TRY(c, c->dx_lsamp.reserve((size_t)lines * 8));
    HIP_TRY(c, hipMemsetAsync(c->dx_pend.p, 0, (size_t)kDemuxSlots * sizeof(DemuxPend), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dx_state.p, 0, 16, c->stream));
    const DtokArgs a = dtok_args(c);
    const DemuxArgs d = demux_args(c);
    const dim3 grid((lines + kDtokThreads - 1) / kDtokThreads);
    KernelTimer* kt = ktimer_begin(c, "demux_lookup");
    {
        const int rc = reads_runs_once(c, a, grid);
        if (rc) return rc;
    }
    if (c->dt_extra)
        hipLaunchKernelGGL(demux_lookup_kernel<true>, grid, dim3(kDtokThreads), 0, c->stream, a, d);
    else
        hipLaunchKernelGGL(demux_lookup_kernel<false>, grid, dim3(kDtokThreads), 0, c->stream, a, d);
    hipLaunchKernelGGL(demux_verify_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, d);
    ktimer_end(c, kt);  // (the launches alone: the waits below are the host's)
    HIP_TRY(c, hipGetLastError());
    uint32_t st[4] = {0, 0, 0, 0};
    DtokState ds{};
    for (uint32_t round = 0;; ++round) {
        HIP_TRY(c, small_back(c, 2, c->dx_state.p, 16));
        if (round == 0) HIP_TRY(c, small_back(c, 0, c->d_state.p, sizeof ds));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        small_back_get(c, 2, st, 16);
        if (round == 0) small_back_get(c, 0, &ds, sizeof ds);
        if (st[0] || ds.flags || st[2] == 0u) break;
        // (names that share a hash with another name: each claims the next slot of its probe, one round per such name)
        if (round > kDemuxMaxSamples) return fail(c, WK_E_STATE, "the pending sample names do not settle");
        kt = ktimer_begin(c, "demux_reclaim");  // (the last round's time is the one kept)
        hipLaunchKernelGGL(store_u32_kernel, dim3(1), dim3(1), 0, c->stream, c->dx_state.as<uint32_t>() + 2, 0u);
        hipLaunchKernelGGL(demux_reclaim_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, d);
        hipLaunchKernelGGL(demux_verify_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, d);
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
    }
    c->dx_looked = true;
    if (st[0] & kDemuxFull) {
        c->dx_status = 1;
        return WK_OK;
    }
    if (st[0] || ds.flags) {  // (a name the host has not mapped, dtok_submap_kernel: the host tokenizer's block)
        c->dx_status = 2;
        return WK_OK;
    }
    const uint32_t n = st[1];
    if (n > d.max_new || n > kDemuxMaxSamples) {
        c->dx_status = 1;
        return WK_OK;
    }
    c->dx_status = 0;
    if (n == 0) return WK_OK;
    HIP_TRY(c, c->dx_out.reserve((size_t)n * sizeof(uint4)));
    hipLaunchKernelGGL(demux_pending_kernel, dim3((n + kDtokThreads - 1) / kDtokThreads), dim3(kDtokThreads), 0, c->stream, a, d, n,
                       c->dx_out.as<uint4>());
    HIP_TRY(c, hipGetLastError());
    std::vector<uint4> got(n);
    HIP_TRY(c, hipMemcpyAsync(got.data(), c->dx_out.p, (size_t)n * sizeof(uint4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::sort(got.begin(), got.end(), [](const uint4& x, const uint4& y) { return x.x < y.x; });
    size_t total = 0;
    for (const uint4& g : got) {
        if ((size_t)g.y + g.z > (size_t)c->dt_n) return fail(c, WK_E_STATE, "a pending sample name lies outside the block");
        c->dx_pend_off.push_back((int64_t)total);
        c->dx_pend_len.push_back((int32_t)g.z);
        total += g.z;
    }
    c->dx_pend_blob.resize(total);
    // the names' bytes come back from the device (the host's bytes of a block copied ahead may be gone): one by one
    // while they are few, with the whole block otherwise
    if (!c->dt_text) return fail(c, WK_E_STATE, "the scanned block's text has been dropped");
    if (n > 128u) {
        std::vector<char> back(c->dt_n);
        HIP_TRY(c, hipMemcpyAsync(back.data(), c->dt_text, c->dt_n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < got.size(); ++k)
            if (got[k].z) std::memcpy(c->dx_pend_blob.data() + c->dx_pend_off[k], back.data() + got[k].y, got[k].z);
    } else {
        for (size_t k = 0; k < got.size(); ++k)
            if (got[k].z)
                HIP_TRY(c, hipMemcpyAsync(c->dx_pend_blob.data() + c->dx_pend_off[k], c->dt_text + got[k].y, got[k].z, hipMemcpyDeviceToHost,
                                          c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return WK_OK;
}

int wk_demux_pending(wk_ctx* c, int64_t* off, int32_t* len, int32_t cap, int32_t* n, char* blob, int64_t blob_cap, int64_t* n_bytes,
                     int* status) {
    if (!c || !n || !n_bytes || !status || cap < 0 || blob_cap < 0) return WK_E_ARG;
    *n = 0;
    *n_bytes = 0;
    *status = 1;
    if (!c->dx_on) return fail(c, WK_E_STATE, "wk_demux_begin has not been called");
    if (!c->dx_looked) {
        // (either flavour: the "ex" flavour's block goes on to wk_dtok_stage_hits_demux)
        if (!c->dt_ready) return fail(c, WK_E_STATE, "no block scanned (wk_dtok_scan)");
        const int rc = demux_lookup(c);
        if (rc) return rc;
    }
    *status = c->dx_status;
    *n = (int32_t)c->dx_pend_off.size();
    *n_bytes = (int64_t)c->dx_pend_blob.size();
    if (!off && !len && !blob) return WK_OK;
    if (!off || !len || cap < *n || (*n_bytes > 0 && (!blob || blob_cap < *n_bytes))) return fail(c, WK_E_CAPACITY, "pending sample buffers too small");
    std::copy(c->dx_pend_off.begin(), c->dx_pend_off.end(), off);
    std::copy(c->dx_pend_len.begin(), c->dx_pend_len.end(), len);
    if (*n_bytes) std::memcpy(blob, c->dx_pend_blob.data(), (size_t)*n_bytes);
    return WK_OK;
}

int wk_demux_register(wk_ctx* c, const char* blob, const int64_t* off, int32_t n, const int32_t* group, int32_t n_total) {
    if (!c || n < 0 || n_total < 0 || (n > 0 && (!off || !blob)) || (n_total > 0 && !group)) return WK_E_ARG;
    if (!c->dx_on) return fail(c, WK_E_STATE, "wk_demux_begin has not been called");
    const size_t known = c->dx_name_off_host.size();
    if (known + (size_t)n > demux_max(c)) return fail(c, WK_E_CAPACITY, "more than %u samples", demux_max(c));
    if ((size_t)n_total != known + (size_t)n) return fail(c, WK_E_ARG, "a group for every sample of the table: %zu", known + (size_t)n);
    for (int32_t i = 0; i < n_total; ++i)
        if (group[i] < -1 || group[i] >= (1 << WK_KEY_GROUP_BITS)) return fail(c, WK_E_ARG, "group id outside [-1, %d)", 1 << WK_KEY_GROUP_BITS);
    for (int32_t k = 0; k < n; ++k) {
        if (off[k] < 0 || off[k + 1] < off[k] || off[k + 1] - off[k] >= (1ll << 28)) return fail(c, WK_E_ARG, "bad name offsets");
        const unsigned char* p = reinterpret_cast<const unsigned char*>(blob) + off[k];
        const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
        const unsigned long long h = demux_hash_of(c->dx_hash_mask, p, len);  // (the kernels' own hash)
        uint32_t q = demux_home(h);
        while (c->dx_tab_host[q].hash != 0ull) {
            if (c->dx_tab_host[q].hash == h) {
                const uint2 nm = c->dx_name_off_host[c->dx_tab_host[q].id];
                if (nm.y == len && (len == 0 || !std::memcmp(c->dx_arena_host.data() + nm.x, p, len)))
                    return fail(c, WK_E_ARG, "sample name %d is in the table already", k);
            }
            q = (q + 1u) & (kDemuxSlots - 1u);
        }
        c->dx_tab_host[q] = DemuxSlot{h, (uint32_t)c->dx_name_off_host.size(), 0u};
        c->dx_name_off_host.push_back(make_uint2((uint32_t)c->dx_arena_host.size(), len));
        c->dx_arena_host.insert(c->dx_arena_host.end(), p, p + len);
    }
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a kernel may be reading the tables that are there)
    int rc;
    if (n > 0) {
        if ((rc = upload(c, c->dx_tab, c->dx_tab_host.data(), c->dx_tab_host.size() * sizeof(DemuxSlot)))) return rc;
        if ((rc = upload(c, c->dx_name_off, c->dx_name_off_host.data(), c->dx_name_off_host.size() * sizeof(uint2)))) return rc;
        if ((rc = upload(c, c->dx_arena, c->dx_arena_host.data(), c->dx_arena_host.size()))) return rc;
    }
    if ((rc = upload(c, c->dx_group, group, (size_t)n_total * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->dx_groups_n = n_total;
    if (n > 0) c->dx_looked = false;  // (the pending names are in the table now)
    return WK_OK;
}

enum StageReads { kStageDemux = 0, kStageStrata = 1, kStagePlain = 2, kStageDemuxKeep = 3 };
static int stage_reads_chunk(wk_ctx* c, StageReads how, int64_t* n_reads, int64_t* n_records, int* status);

// wk_dtok_stage_reads / wk_dtok_stage_reads_samples: the checks, the lookup of the samples if it has not run, the chunk
static int stage_reads_demux(wk_ctx* c, StageReads how, int64_t* n_reads, int64_t* n_records, int* status) {
    if (!c || !n_reads || !n_records || !status) return WK_E_ARG;
    *status = 1;
    *n_reads = *n_records = 0;
    if (!c->dx_on) return fail(c, WK_E_STATE, "wk_demux_begin has not been called");
    if (!c->dt_ready || c->dt_extra) return fail(c, WK_E_STATE, "no block scanned for the plain flavour (wk_dtok_scan)");
    if (c->dx_groups_n != (int32_t)c->dx_name_off_host.size()) return fail(c, WK_E_STATE, "samples without a group (wk_demux_register)");
    if (c->acc_open) return fail(c, WK_E_STATE, "staged hits not counted yet (wk_ordinal_count)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    // (run starts, subject map, exclusion set: wk_demux_pending has done them, or does now)
    if (!c->dx_looked || c->dx_status != 0 || !c->dx_pend_off.empty()) {
        if (!c->dx_looked) {
            const int rc = demux_lookup(c);
            if (rc) return rc;
        }
        if (c->dx_status != 0) {
            c->dt_ready = false;
            return WK_OK;
        }
        if (!c->dx_pend_off.empty()) return fail(c, WK_E_STATE, "the block brings samples the table does not hold (wk_demux_pending, wk_demux_register)");
    }
    return stage_reads_chunk(c, how, n_reads, n_records, status);
}

int wk_dtok_stage_reads(wk_ctx* c, int64_t* n_reads, int64_t* n_records, int* status) {
    return stage_reads_demux(c, kStageDemux, n_reads, n_records, status);
}

// The block scanned last for the plain flavour as the staged CSR chunk with a group per read: the group of the read's
// sample (wk_demux.hpp; the samples have been looked up) or, `strata`, of its stratum in the map that is loaded
// (wk_strata_reads.hpp) -- or, kStagePlain, with no group per read at all: the caller names the one group of all of
// them (wk_set_uniform_group), and the reads' leader lines are kept for wk_dtok_readmap_reads (wk_readmap_reads.hpp).
// *status stays 1 for a block the kernels leave to the host tokenizer.
static int stage_reads_chunk(wk_ctx* c, StageReads how, int64_t* n_reads, int64_t* n_records, int* status) {
    const bool keep = how == kStageDemuxKeep;  // (the reads' sample ids and leader lines are kept: wk_readmap_demux.hpp)
    const bool strata = how != kStageDemux && !keep;  // (run starts told here; no samples to look up)
    const bool plain = how == kStagePlain;
    c->dt_ready = false;
    c->dx_looked = false;
    c->chunk_valid = false;
    c->dx_chunk = false;
    c->rr_chunk = false;
    c->rd_chunk = false;
    c->dx_hits = false;
    const uint32_t lines = c->dt_lines;
    const size_t n_samples = strata ? 0 : c->dx_name_off_host.size();
    if (n_samples) HIP_TRY(c, hipMemsetAsync(c->dx_met.p, 0, n_samples, c->stream));
    unsigned long long totals = 0;
    uint32_t st[4] = {0, 0, 0, 0};
    DtokState ds{};
    HIP_TRY(c, c->c_subj.reserve((size_t)lines * 4 + 64));
    HIP_TRY(c, c->c_qoff.reserve(((size_t)lines + 2) * 4));
    HIP_TRY(c, c->c_group.reserve(((size_t)lines + 1) * 4));
    if (keep) HIP_TRY(c, c->rd_samp.reserve(((size_t)lines + 1) * 4));
    if (lines > 0) {
        DtokArgs a = dtok_args(c);
        const uint32_t n_tiles = (lines + kDtokThreads - 1) / kDtokThreads;
        HIP_TRY(c, c->d_tiles.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, c->d_tile_off.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, c->d_lscan.reserve(((size_t)lines + 1) * 8));
        a.line_scan = c->d_lscan.as<unsigned long long>();
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
        if (!strata) HIP_TRY(c, hipMemsetAsync(c->dx_state.p, 0, 16, c->stream));
        const dim3 grid(n_tiles);
        KernelTimer* kt = ktimer_begin(c, plain ? "reads_stage" : strata ? "strata_stage" : "demux_stage");
        if (strata) {  // (under `--demux` the lookup of the samples has told the runs)
            const int rc = reads_runs_once(c, a, grid);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(dtok_first_kernel, grid, dim3(kDtokThreads), 0, c->stream, a);
        hipLaunchKernelGGL(dtok_hits_kernel<false>, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tiles.as<unsigned long long>());
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                           c->d_tile_off.as<unsigned long long>(), (int64_t)n_tiles, scalar_u64(c, 3));
        hipLaunchKernelGGL(dtok_scan_lines_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tile_off.as<unsigned long long>());
        if (strata) {
            const StrataChunk ch{c->c_subj.as<int32_t>(), c->c_qoff.as<int32_t>(), c->c_group.as<int32_t>(), lines};
            if (plain)
                hipLaunchKernelGGL(strata_place_reads_kernel<false>, grid, dim3(kDtokThreads), 0, c->stream, a, StrataArgs{}, ch);
            else
                hipLaunchKernelGGL(strata_place_reads_kernel<true>, grid, dim3(kDtokThreads), 0, c->stream, a, strata_args(c), ch);
        } else {
            DemuxArgs d = demux_args(c);
            d.c_subj = c->c_subj.as<int32_t>();
            d.c_qoff = c->c_qoff.as<int32_t>();
            d.c_group = c->c_group.as<int32_t>();
            d.cap = lines;
            hipLaunchKernelGGL(demux_place_reads_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, d, keep ? c->rd_samp.as<int32_t>() : nullptr);
        }
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, small_back(c, 0, c->d_state.p, sizeof ds));
        HIP_TRY(c, small_back(c, 1, scalar_u64(c, 3), 8));
        if (!strata) HIP_TRY(c, small_back(c, 2, c->dx_state.p, 16));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        small_back_get(c, 0, &ds, sizeof ds);
        small_back_get(c, 1, &totals, 8);
        if (!strata) small_back_get(c, 2, st, 16);
    }
    // (a read of more than WK_MAX_K subjects, a name the host has not mapped: the host tokenizer's block)
    if (ds.flags || st[0]) return WK_OK;
    const int64_t records = (int64_t)(totals & 0xFFFFFFFFull), reads = (int64_t)(totals >> 32);
    if (records > (int64_t)lines || reads > records) return fail(c, WK_E_STATE, "the block's reads do not add up");
    // (the offsets' last entry; the stream orders it in front of whatever reads them)
    hipLaunchKernelGGL(store_u32_kernel, dim3(1), dim3(1), 0, c->stream, c->c_qoff.as<uint32_t>() + reads, (uint32_t)records);
    HIP_TRY(c, hipGetLastError());
    c->rk_valid[0] = c->rk_valid[1] = false;
    c->stage_serial += 1;
    c->cur_subj = c->c_subj.as<int32_t>();
    c->cur_qoff = c->c_qoff.as<int32_t>();
    if ((plain || keep) && reads > 0) {
        // the leader line of every read, in the chunk's read order (a read no leader names keeps "no line")
        HIP_TRY(c, c->rm_line.reserve((size_t)reads * 4));
        HIP_TRY(c, hipMemsetAsync(c->rm_line.p, 0xFF, (size_t)reads * 4, c->stream));
        DtokArgs a = dtok_args(c);
        a.line_scan = c->d_lscan.as<unsigned long long>();
        hipLaunchKernelGGL(readmap_leaders_kernel, dim3((lines + kDtokThreads - 1) / kDtokThreads), dim3(kDtokThreads), 0, c->stream, a,
                           c->rm_line.as<uint32_t>(), (uint32_t)reads);
        HIP_TRY(c, hipGetLastError());
    }
    c->n_reads = reads;
    c->n_records = records;
    c->has_group = !plain;
    c->group_base = 0;
    c->subj_is_set = true;
    c->subj_indexed = true;
    c->chunk_valid = true;
    c->dx_chunk = !plain;
    c->rr_chunk = plain;
    c->rd_chunk = keep;
    *n_reads = reads;
    *n_records = records;
    *status = 0;
    return WK_OK;
}

int wk_demux_fetch(wk_ctx* c, int32_t* group, int64_t group_cap, unsigned char* met, int32_t met_cap) {
    if (!c || group_cap < 0 || met_cap < 0) return WK_E_ARG;
    if (!c->dx_on) return fail(c, WK_E_STATE, "wk_demux_begin has not been called");
    if (!(c->dx_chunk || c->dx_hits) || !c->chunk_valid)
        return fail(c, WK_E_STATE, "no chunk staged by wk_dtok_stage_reads, none matched behind wk_dtok_stage_hits_demux");
    const size_t n_samples = c->dx_name_off_host.size();
    if ((group && group_cap < c->n_reads) || (met && (size_t)met_cap < n_samples)) return fail(c, WK_E_CAPACITY, "fetch buffers too small");
    DeviceGuard guard(c->device);
    if (group && c->n_reads) HIP_TRY(c, hipMemcpyAsync(group, c->c_group.p, (size_t)c->n_reads * 4, hipMemcpyDeviceToHost, c->stream));
    if (met && n_samples) HIP_TRY(c, hipMemcpyAsync(met, c->dx_met.p, n_samples, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// The block scanned last for the "ex" flavour as the staged hits of the coord-match, a read's group its sample's
// (demux_place_hits_kernel).  *status stays 1 for a block the host tokenizer takes.
int wk_dtok_stage_hits_demux(wk_ctx* c, const int32_t* genome_of_subject, int32_t n_subjects, double th, int64_t* n_reads, int64_t* n_hits,
                             int* status) {
    if (!c || !n_reads || !n_hits || !status || n_subjects < 0 || (n_subjects > 0 && !genome_of_subject)) return WK_E_ARG;
    *status = 1;
    *n_reads = *n_hits = 0;
    if (!c->dx_on) return fail(c, WK_E_STATE, "wk_demux_begin has not been called");
    if (!c->dt_ready || !c->dt_extra) return fail(c, WK_E_STATE, "no block scanned for the \"ex\" flavour (wk_dtok_scan)");
    if (!(th > 0.0)) return fail(c, WK_E_ARG, "overlap threshold must be positive");
    if (c->dx_groups_n != (int32_t)c->dx_name_off_host.size()) return fail(c, WK_E_STATE, "samples without a group (wk_demux_register)");
    if (c->acc_open) return fail(c, WK_E_STATE, "staged hits not counted yet (wk_ordinal_count)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    if (!c->dx_looked) {
        const int rc = demux_lookup(c);
        if (rc) return rc;
    }
    if (c->dx_status != 0) {
        c->dt_ready = false;
        return WK_OK;
    }
    if (!c->dx_pend_off.empty()) return fail(c, WK_E_STATE, "the block brings samples the table does not hold (wk_demux_pending, wk_demux_register)");
    c->dt_ready = false;
    c->dx_looked = false;
    c->chunk_valid = false;
    c->dx_chunk = false;
    c->rr_chunk = false;
    c->rd_chunk = false;
    c->dx_hits = false;
    c->ord_valid = false;
    const uint32_t lines = c->dt_lines;
    if ((int64_t)lines >= (1ll << 31) - 64) return fail(c, WK_E_RANGE, "more than 2^31 hits staged");
    const size_t n_samples = c->dx_name_off_host.size();
    if (n_samples) HIP_TRY(c, hipMemsetAsync(c->dx_met.p, 0, n_samples, c->stream));
    int rc;
    if ((rc = upload(c, c->d_gmap, genome_of_subject, (size_t)std::max(n_subjects, 1) * 4))) return rc;
    const size_t cap_h = (size_t)lines + 1;
    HIP_TRY(c, c->o_genome.reserve(cap_h * 4));
    HIP_TRY(c, c->o_beg.reserve(cap_h * 4));
    HIP_TRY(c, c->o_end.reserve(cap_h * 4));
    HIP_TRY(c, c->o_len.reserve(cap_h * 4));
    HIP_TRY(c, c->o_hoff.reserve(((size_t)lines + 2) * 4));
    HIP_TRY(c, c->c_group.reserve(((size_t)lines + 1) * 4));
    HIP_TRY(c, c->dx_rsamp.reserve(((size_t)lines + 1) * 4));
    unsigned long long totals = 0;
    uint32_t st[4] = {0, 0, 0, 0};
    DtokState ds{};
    if (lines > 0) {
        DtokArgs a = dtok_args(c);
        a.gmap = c->d_gmap.as<int32_t>();
        a.n_gmap = (uint32_t)n_subjects;
        a.o_genome = c->o_genome.as<int32_t>();
        a.o_beg = c->o_beg.as<int32_t>();
        a.o_end = c->o_end.as<int32_t>();
        a.o_len = c->o_len.as<uint32_t>();
        a.o_hoff = c->o_hoff.as<int32_t>();
        a.o_hit_base = 0u;
        const uint32_t n_tiles = (lines + kDtokThreads - 1) / kDtokThreads;
        HIP_TRY(c, c->d_tiles.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, c->d_tile_off.reserve((size_t)n_tiles * 8));
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->dx_state.p, 0, 16, c->stream));
        DemuxArgs d = demux_args(c);
        d.c_group = c->c_group.as<int32_t>();
        d.cap = lines;
        const dim3 grid(n_tiles);
        KernelTimer* kt = ktimer_begin(c, "demux_stage_hits");
        if ((rc = reads_runs_once(c, a, grid))) return rc;  // (the lookup of the samples has told the runs)
        hipLaunchKernelGGL(dtok_hits_kernel<true>, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tiles.as<unsigned long long>());
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                           c->d_tile_off.as<unsigned long long>(), (int64_t)n_tiles, scalar_u64(c, 3));
        hipLaunchKernelGGL(dtok_scan_lines_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, c->d_tile_off.as<unsigned long long>());
        hipLaunchKernelGGL(demux_place_hits_kernel, grid, dim3(kDtokThreads), 0, c->stream, a, d, c->dx_rsamp.as<int32_t>());
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, small_back(c, 0, c->d_state.p, sizeof ds));
        HIP_TRY(c, small_back(c, 1, scalar_u64(c, 3), 8));
        HIP_TRY(c, small_back(c, 2, c->dx_state.p, 16));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        small_back_get(c, 0, &ds, sizeof ds);
        small_back_get(c, 1, &totals, 8);
        small_back_get(c, 2, st, 16);
    }
    // (a full table, a name that is not registered, a flag of the scan's: the host tokenizer's block)
    if (ds.flags || st[0]) return WK_OK;
    const int64_t hits = (int64_t)(totals & 0xFFFFFFFFull), reads = (int64_t)(totals >> 32);
    if (hits > (int64_t)lines || reads > hits) return fail(c, WK_E_STATE, "the block's hits do not add up");
    // (the offsets' last entry; the stream orders it in front of whatever reads them)
    hipLaunchKernelGGL(store_u32_kernel, dim3(1), dim3(1), 0, c->stream, c->o_hoff.as<uint32_t>() + reads, (uint32_t)hits);
    HIP_TRY(c, hipGetLastError());
    c->n_hits = hits;
    c->o_reads = reads;
    c->th = th;
    c->has_group = true;
    c->group_base = 0;
    c->rk_valid[0] = c->rk_valid[1] = false;
    c->ord_valid = true;
    c->sb_valid = false;
    c->acc_open = false;
    c->dx_hits = true;
    *n_reads = reads;
    *n_hits = hits;
    *status = 0;
    return WK_OK;
}

// ---- plain classification with a strata map on the device (wk_strata_reads.hpp) -------------------------------------

int wk_dtok_stage_reads_strata(wk_ctx* c, int64_t* n_reads, int64_t* n_records, int* status) {
    if (!c || !n_reads || !n_records || !status) return WK_E_ARG;
    *status = 1;
    *n_reads = *n_records = 0;
    if (!c->s_ready || !c->s_use) return fail(c, WK_E_STATE, "no strata map with groups on the device (wk_strata_load, wk_strata_groups)");
    if (c->dx_on) return fail(c, WK_E_STATE, "the reads' groups are their samples' (wk_demux_begin): wk_dtok_stage_reads");
    if (!c->dt_ready || c->dt_extra) return fail(c, WK_E_STATE, "no block scanned for the plain flavour (wk_dtok_scan)");
    if (c->acc_open) return fail(c, WK_E_STATE, "staged hits not counted yet (wk_ordinal_count)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    return stage_reads_chunk(c, kStageStrata, n_reads, n_records, status);
}

int wk_chunk_groups(wk_ctx* c, int32_t* group, int64_t cap) {
    if (!c || cap < 0 || (cap > 0 && !group)) return WK_E_ARG;
    if (!c->dx_chunk || !c->chunk_valid) return fail(c, WK_E_STATE, "no chunk staged by wk_dtok_stage_reads / wk_dtok_stage_reads_strata");
    if (cap < c->n_reads) return fail(c, WK_E_CAPACITY, "need room for %lld groups", (long long)c->n_reads);
    DeviceGuard guard(c->device);
    if (c->n_reads) HIP_TRY(c, hipMemcpyAsync(group, c->c_group.p, (size_t)c->n_reads * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// ---- read maps of whole-read assignments on the device (wk_readmap_reads.hpp) ------------------------------------

int wk_dtok_stage_reads_plain(wk_ctx* c, int64_t* n_reads, int64_t* n_records, int* status) {
    if (!c || !n_reads || !n_records || !status) return WK_E_ARG;
    *status = 1;
    *n_reads = *n_records = 0;
    if (c->dx_on) return fail(c, WK_E_STATE, "the reads' groups are their samples' (wk_demux_begin): wk_dtok_stage_reads");
    if (!c->dt_ready || c->dt_extra) return fail(c, WK_E_STATE, "no block scanned for the plain flavour (wk_dtok_scan)");
    if (c->acc_open) return fail(c, WK_E_STATE, "staged hits not counted yet (wk_ordinal_count)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    return stage_reads_chunk(c, kStagePlain, n_reads, n_records, status);
}

// A text table over the feature ids (features [first, first + n) hold text[off[k], off[k + 1])): set from 0 or extended
// from its size `have`, whose text ends at `have_text`.
static int text_table_set(wk_ctx* c, const char* what, DevBuf& d_off, DevBuf& d_text, int32_t& have, uint32_t& have_text, int32_t first, int32_t n,
                          const uint32_t* shown_off, const char* shown) {
    if (first < 0 || n < 0 || (n > 0 && !shown_off)) return fail(c, WK_E_ARG, "bad %s table", what);
    if (first != 0 && first != have) return fail(c, WK_E_ARG, "the %s table holds %d features: set it from 0 or extend it from there", what, have);
    if (n > 0 && shown_off[0] != 0) return fail(c, WK_E_ARG, "shown_off must start at 0");
    for (int32_t k = 0; k < n; ++k)
        if (shown_off[k + 1] < shown_off[k]) return fail(c, WK_E_ARG, "shown_off must not decrease");
    const uint32_t n_text = n > 0 ? shown_off[n] : 0u;
    if (n_text > 0 && !shown) return fail(c, WK_E_ARG, "bad %s table", what);
    const uint32_t base = first ? have_text : 0u;
    if ((uint64_t)base + n_text >= (1ull << 32) || (int64_t)first + n >= (1ll << 31)) return fail(c, WK_E_RANGE, "%s table beyond 2^32 bytes", what);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a kernel may be reading the table that is there)
    HIP_TRY(c, grow_keep(c, d_off, ((size_t)first + n + 1) * 4, first ? ((size_t)first + 1) * 4 : 0));
    HIP_TRY(c, grow_keep(c, d_text, (size_t)base + n_text + 64, base));
    std::vector<uint32_t> off((size_t)n + 1);
    for (int32_t k = 0; k <= n; ++k) off[k] = base + (n > 0 ? shown_off[k] : 0u);
    HIP_TRY(c, hipMemcpyAsync(d_off.as<uint32_t>() + first, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (n_text) HIP_TRY(c, hipMemcpyAsync(d_text.as<unsigned char>() + base, shown, n_text, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's buffers are only valid during the call)
    have = first + n;
    have_text = base + n_text;
    return WK_OK;
}

int wk_readmap_reads_tables(wk_ctx* c, int32_t first, int32_t n, const uint32_t* shown_off, const char* shown) {
    if (!c) return WK_E_ARG;
    const int rc = text_table_set(c, "shown-text", c->rr_off, c->rr_text, c->rr_n, c->rr_text_n, first, n, shown_off, shown);
    if (rc == WK_OK && first == 0) c->rl_n = 0;  // (a new table: the ids of the one before say nothing about it)
    return rc;
}

int wk_readmap_lists_ids(wk_ctx* c, int32_t first, int32_t n, const uint32_t* id_off, const char* ids) {
    if (!c) return WK_E_ARG;
    return text_table_set(c, "id", c->rl_off, c->rl_text, c->rl_n, c->rl_text_n, first, n, id_off, ids);
}

int wk_dtok_readmap_reads(wk_ctx* c, int32_t job, int64_t* n_bytes) {
    if (!c || !n_bytes) return WK_E_ARG;
    *n_bytes = 0;
    c->rm_bytes = 0;
    if (!c->rr_chunk || !c->chunk_valid) return fail(c, WK_E_STATE, "no chunk staged by wk_dtok_stage_reads_plain");
    if (c->rr_serial != c->stage_serial) return fail(c, WK_E_STATE, "the staged chunk's codes are not on the device (wk_classify_staged_keep)");
    if (job < 0 || job >= c->rr_jobs) return fail(c, WK_E_ARG, "job must be in [0, %d)", c->rr_jobs);
    if (c->n_reads >= (1ll << 32) - 1) return fail(c, WK_E_RANGE, "more than 2^32 reads in one block");
    const uint32_t n_reads = (uint32_t)c->n_reads;
    if (n_reads == 0 || c->dt_lines == 0) return WK_OK;
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    HIP_TRY(c, c->rm_len.reserve((size_t)n_reads * 8));
    HIP_TRY(c, c->rr_flags.reserve(16));
    HIP_TRY(c, c->rr_off.reserve(4));  // (an empty table still has its first offset's place)
    DtokArgs a = dtok_args(c);
    ReadmapReadsArgs m{};
    m.assign = c->assign_out.as<int32_t>() + (size_t)job * n_reads;
    m.read_line = c->rm_line.as<uint32_t>();
    m.shown_off = c->rr_off.as<uint32_t>();
    m.shown = c->rr_text.as<unsigned char>();
    m.n_shown = (uint32_t)c->rr_n;
    m.read_len = c->rm_len.as<unsigned long long>();
    m.flags = c->rr_flags.as<uint32_t>();
    m.n_reads = n_reads;
    m.unassigned = c->rr_unassigned;
    const dim3 rgrid((n_reads + kDtokThreads - 1) / kDtokThreads);
    HIP_TRY(c, c->d_tiles.reserve((size_t)rgrid.x * 8));
    HIP_TRY(c, c->d_tile_off.reserve((size_t)rgrid.x * 8));
    HIP_TRY(c, hipMemsetAsync(c->rr_flags.p, 0, 16, c->stream));
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
    KernelTimer* kt = ktimer_begin(c, "readmap_reads");
    hipLaunchKernelGGL(readmap_reads_len_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, m);
    hipLaunchKernelGGL(u64_tile_sum_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, m.read_len, n_reads, c->d_tiles.as<unsigned long long>());
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                       c->d_tile_off.as<unsigned long long>(), (int64_t)rgrid.x, scalar_u64(c, 3));
    hipLaunchKernelGGL(u64_tile_prefix_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, m.read_len, n_reads, c->d_tile_off.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    unsigned long long total = 0;
    uint32_t flags = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&flags, c->rr_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (flags) {
        ktimer_end(c, kt);
        return fail(c, WK_E_STATE, "job %d left a code that is no single feature of the shown-text table (%d features)", job, c->rr_n);
    }
    if (total >= (1ull << 40)) return fail(c, WK_E_RANGE, "read-map text of one block beyond 2^40 bytes");
    if (total > 0) {
        HIP_TRY(c, c->rm_text.reserve((size_t)total + 64));
        m.out = c->rm_text.as<unsigned char>();
        m.out_cap = total;
        hipLaunchKernelGGL(readmap_reads_write_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, m);
        HIP_TRY(c, hipGetLastError());
    }
    ktimer_end(c, kt);
    c->rm_bytes = (int64_t)total;
    *n_bytes = (int64_t)total;
    return WK_OK;
}

// ---- read maps with taxon lists on the device (wk_readmap_lists.hpp) ---------------------------------------------

int wk_dtok_readmap_lists(wk_ctx* c, int32_t job, int64_t* n_bytes) {
    if (!c || !n_bytes) return WK_E_ARG;
    *n_bytes = 0;
    c->rm_bytes = 0;
    if (!c->rr_chunk || !c->chunk_valid) return fail(c, WK_E_STATE, "no chunk staged by wk_dtok_stage_reads_plain");
    if (c->rr_serial != c->stage_serial) return fail(c, WK_E_STATE, "the staged chunk's codes are not on the device (wk_classify_staged_keep)");
    if (job < 0 || job >= c->rr_jobs) return fail(c, WK_E_ARG, "job must be in [0, %d)", c->rr_jobs);
    if (c->n_reads >= (1ll << 32) - 1 || c->n_records >= (1ll << 31)) return fail(c, WK_E_RANGE, "more than 2^31 records in one block");
    if (c->rl_n != 0 && c->rl_n != c->rr_n)
        return fail(c, WK_E_STATE, "the id table holds %d features, the shown-text table %d (wk_readmap_lists_ids)", c->rl_n, c->rr_n);
    const uint32_t n_reads = (uint32_t)c->n_reads;
    if (n_reads == 0 || c->dt_lines == 0) return WK_OK;
    const int32_t* anc = nullptr;
    if (c->rl_mode[job] == WK_MODE_RANK) {
        const int slot = c->rl_slot[job];
        if (slot < 0 || slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) || !c->rank_tab_valid[slot])
            return fail(c, WK_E_STATE, "job %d: rank slot %d has not been built", job, slot);
        anc = c->rank_tab[slot].as<int32_t>();
    }
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    HIP_TRY(c, c->rm_len.reserve((size_t)n_reads * 8));
    HIP_TRY(c, c->rr_flags.reserve(16));
    HIP_TRY(c, c->rr_off.reserve(4));  // (an empty table still has its first offset's place)
    HIP_TRY(c, c->rl_pairs.reserve((size_t)std::max<int64_t>(c->n_records, 1) * sizeof(uint2)));
    HIP_TRY(c, c->rl_npairs.reserve((size_t)n_reads * 4));
    DtokArgs a = dtok_args(c);
    ReadmapListsArgs L{};
    ReadmapReadsArgs& m = L.m;
    m.assign = c->assign_out.as<int32_t>() + (size_t)job * n_reads;
    m.read_line = c->rm_line.as<uint32_t>();
    m.shown_off = c->rr_off.as<uint32_t>();
    m.shown = c->rr_text.as<unsigned char>();
    m.n_shown = (uint32_t)c->rr_n;
    m.read_len = c->rm_len.as<unsigned long long>();
    m.flags = c->rr_flags.as<uint32_t>();
    m.n_reads = n_reads;
    m.unassigned = c->rr_unassigned;
    L.subj = c->cur_subj;
    L.qoff = c->cur_qoff;
    L.subj_feat = c->subj_feat.as<int32_t>();
    L.n_subjects = (uint32_t)std::max(c->n_subjects, 0);
    L.anc = anc;
    L.n_nodes = (uint32_t)std::max(c->n_nodes, 0);
    L.key_off = c->rl_n ? c->rl_off.as<uint32_t>() : m.shown_off;
    L.key = c->rl_n ? c->rl_text.as<unsigned char>() : m.shown;
    L.pairs = c->rl_pairs.as<uint2>();
    L.n_pairs = c->rl_npairs.as<uint32_t>();
    const dim3 rgrid((n_reads + kDtokThreads - 1) / kDtokThreads);
    HIP_TRY(c, c->d_tiles.reserve((size_t)rgrid.x * 8));
    HIP_TRY(c, c->d_tile_off.reserve((size_t)rgrid.x * 8));
    HIP_TRY(c, hipMemsetAsync(c->rr_flags.p, 0, 16, c->stream));
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
    KernelTimer* kt = ktimer_begin(c, "readmap_lists");
    hipLaunchKernelGGL(readmap_lists_build_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, L);
    hipLaunchKernelGGL(u64_tile_sum_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, m.read_len, n_reads, c->d_tiles.as<unsigned long long>());
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_tiles.as<unsigned long long>(),
                       c->d_tile_off.as<unsigned long long>(), (int64_t)rgrid.x, scalar_u64(c, 3));
    hipLaunchKernelGGL(u64_tile_prefix_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, m.read_len, n_reads, c->d_tile_off.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    unsigned long long total = 0;
    uint32_t flags = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&flags, c->rr_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (flags) {
        ktimer_end(c, kt);
        return fail(c, WK_E_STATE, "job %d left a code or a list that the tables cannot print (%d features shown, %d subjects)", job, c->rr_n,
                    c->n_subjects);
    }
    if (total >= (1ull << 40)) return fail(c, WK_E_RANGE, "read-map text of one block beyond 2^40 bytes");
    if (total > 0) {
        HIP_TRY(c, c->rm_text.reserve((size_t)total + 64));
        m.out = c->rm_text.as<unsigned char>();
        m.out_cap = total;
        hipLaunchKernelGGL(readmap_lists_write_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, L);
        HIP_TRY(c, hipGetLastError());
    }
    ktimer_end(c, kt);
    c->rm_bytes = (int64_t)total;
    *n_bytes = (int64_t)total;
    return WK_OK;
}

// ---- read maps under demultiplexing on the device (wk_readmap_demux.hpp) -----------------------------------------

static int64_t part_cap(const wk_ctx* c) { return c->pd_cap_opt ? c->pd_cap_opt : kPartCapDefault; }

static PartArgs part_args(wk_ctx* c, const int32_t* samp, uint32_t n) {
    PartArgs p{};
    p.samp = samp;
    p.n = n;
    p.n_tiles = (n + kPartTile - 1) / kPartTile;
    p.present = c->pd_present.as<uint32_t>();
    p.n_cols = c->pd_state.as<uint32_t>();
    p.flags = c->pd_state.as<uint32_t>() + 1;
    p.total = c->pd_state.as<unsigned long long>() + 1;
    p.mat = c->pd_mat.as<unsigned long long>();
    p.col = c->pd_col.as<unsigned long long>();
    p.seg = c->pd_seg.as<unsigned long long>();
    p.off = c->pd_off.as<unsigned long long>();
    return p;
}

// The columns of the samples samp[0, n) (device) holds, the segment table's ids: *n_cols = D.  Waits for the stream.
static int part_columns(wk_ctx* c, const int32_t* samp, uint32_t n, uint32_t* n_cols) {
    *n_cols = 0;
    HIP_TRY(c, c->pd_present.reserve((size_t)kDemuxMaxSamples * 4));
    HIP_TRY(c, c->pd_state.reserve(64));
    HIP_TRY(c, c->pd_col.reserve((size_t)kDemuxMaxSamples * 8));
    HIP_TRY(c, c->pd_seg.reserve((size_t)kDemuxMaxSamples * 3 * 8));
    HIP_TRY(c, hipMemsetAsync(c->pd_present.p, 0, (size_t)kDemuxMaxSamples * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->pd_state.p, 0, 16, c->stream));
    const PartArgs p = part_args(c, samp, n);
    if (n > 0) hipLaunchKernelGGL(readmap_demux_mark_kernel, dim3((n + kDtokThreads - 1) / kDtokThreads), dim3(kDtokThreads), 0, c->stream, p);
    hipLaunchKernelGGL(readmap_demux_rank_kernel, dim3(1), dim3(kPartScanThreads), 0, c->stream, p);
    HIP_TRY(c, hipGetLastError());
    uint32_t st[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(st, c->pd_state.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st[1]) return fail(c, WK_E_RANGE, "a sample id beyond %u", kDemuxMaxSamples);
    if (st[0] > kDemuxMaxSamples) return fail(c, WK_E_STATE, "the samples' columns do not add up");
    *n_cols = st[0];
    return WK_OK;
}

// Behind part_columns: the places off[r] of len[0, n) (device) in pd_off, the segment table, *total.  The caller has
// checked tiles x n_cols against the capacity.  Waits for the stream.
static int part_places(wk_ctx* c, const int32_t* samp, const unsigned long long* len, uint32_t n, uint32_t n_cols, unsigned long long* total) {
    *total = 0;
    if (n == 0 || n_cols == 0) return WK_OK;
    const uint32_t tiles = (n + kPartTile - 1) / kPartTile;
    if ((int64_t)tiles * n_cols > part_cap(c)) return fail(c, WK_E_CAPACITY, "%u tiles x %u samples beyond the partition's matrix", tiles, n_cols);
    HIP_TRY(c, c->pd_mat.reserve((size_t)tiles * n_cols * 8));
    HIP_TRY(c, c->pd_off.reserve((size_t)n * 8));
    HIP_TRY(c, hipMemsetAsync(c->pd_mat.p, 0, (size_t)tiles * n_cols * 8, c->stream));
    PartArgs p = part_args(c, samp, n);
    p.len = len;
    hipLaunchKernelGGL(readmap_demux_tile_kernel, dim3(tiles), dim3(kPartTile), 0, c->stream, p, n_cols);
    hipLaunchKernelGGL(readmap_demux_columns_kernel, dim3((n_cols + kWave - 1) / kWave), dim3(kWave * kPartStrips), 0, c->stream, p, n_cols);
    hipLaunchKernelGGL(readmap_demux_across_kernel, dim3(1), dim3(kPartScanThreads), 0, c->stream, p, n_cols);
    hipLaunchKernelGGL(readmap_demux_add_kernel, dim3((n + kDtokThreads - 1) / kDtokThreads), dim3(kDtokThreads), 0, c->stream, p, n_cols);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(total, p.total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// wk_dtok_stage_reads with the sample id of every read and the reads' leader lines kept, and the samples of the block
// given their columns.  *status = 4: more tiles x samples than the partition's matrix holds -- no chunk is left staged and
// nothing has been counted, the host tokenizer takes the block.  (The placement has run by then: the "met" bytes of the
// block's samples are set on the device.  Nobody fetches them for a refused block -- wk_demux_fetch wants a staged chunk --
// and the next staging clears them; the host route gives the same samples their columns.)
int wk_dtok_stage_reads_samples(wk_ctx* c, int64_t* n_reads, int64_t* n_records, int* status) {
    const int rc = stage_reads_demux(c, kStageDemuxKeep, n_reads, n_records, status);
    if (rc || *status) return rc;
    DeviceGuard guard(c->device);
    c->rd_cols = 0;
    uint32_t cols = 0;
    int rc2 = WK_OK;
    if (*n_reads > 0) rc2 = part_columns(c, c->rd_samp.as<int32_t>(), (uint32_t)*n_reads, &cols);
    const int64_t tiles = (*n_reads + kPartTile - 1) / kPartTile;
    if (rc2 || tiles * (int64_t)cols > part_cap(c)) {
        c->chunk_valid = false;
        c->dx_chunk = false;
        c->rd_chunk = false;
        *n_reads = *n_records = 0;
        *status = 4;
        return rc2;
    }
    c->rd_cols = cols;
    return WK_OK;
}

// wk_dtok_readmap_reads / wk_dtok_readmap_lists under demultiplexing: the text of job `job` over the chunk of
// wk_dtok_stage_reads_samples, one run per sample (*n_segments of them: wk_dtok_readmap_segments).
static int readmap_demux_impl(wk_ctx* c, int32_t job, int64_t* n_bytes, int32_t* n_segments, bool lists) {
    if (!c || !n_bytes || !n_segments) return WK_E_ARG;
    *n_bytes = 0;
    *n_segments = 0;
    c->rm_bytes = 0;
    c->rd_segs = 0;
    if (!c->rd_chunk || !c->chunk_valid) return fail(c, WK_E_STATE, "no chunk staged by wk_dtok_stage_reads_samples");
    if (c->rr_serial != c->stage_serial) return fail(c, WK_E_STATE, "the staged chunk's codes are not on the device (wk_classify_staged_keep)");
    if (job < 0 || job >= c->rr_jobs) return fail(c, WK_E_ARG, "job must be in [0, %d)", c->rr_jobs);
    if (c->n_reads >= (1ll << 32) - 1 || c->n_records >= (1ll << 31)) return fail(c, WK_E_RANGE, "more than 2^31 records in one block");
    if (lists && c->rl_n != 0 && c->rl_n != c->rr_n)
        return fail(c, WK_E_STATE, "the id table holds %d features, the shown-text table %d (wk_readmap_lists_ids)", c->rl_n, c->rr_n);
    const uint32_t n_reads = (uint32_t)c->n_reads;
    if (n_reads == 0 || c->dt_lines == 0 || c->rd_cols == 0) return WK_OK;
    const int32_t* anc = nullptr;
    if (lists && c->rl_mode[job] == WK_MODE_RANK) {
        const int slot = c->rl_slot[job];
        if (slot < 0 || slot >= (int)(sizeof c->rank_tab / sizeof c->rank_tab[0]) || !c->rank_tab_valid[slot])
            return fail(c, WK_E_STATE, "job %d: rank slot %d has not been built", job, slot);
        anc = c->rank_tab[slot].as<int32_t>();
    }
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    HIP_TRY(c, c->rm_len.reserve((size_t)n_reads * 8));
    HIP_TRY(c, c->rr_flags.reserve(16));
    HIP_TRY(c, c->rr_off.reserve(4));  // (an empty table still has its first offset's place)
    if (lists) {
        HIP_TRY(c, c->rl_pairs.reserve((size_t)std::max<int64_t>(c->n_records, 1) * sizeof(uint2)));
        HIP_TRY(c, c->rl_npairs.reserve((size_t)n_reads * 4));
    }
    DtokArgs a = dtok_args(c);
    ReadmapListsArgs L{};
    ReadmapReadsArgs& m = L.m;
    m.assign = c->assign_out.as<int32_t>() + (size_t)job * n_reads;
    m.read_line = c->rm_line.as<uint32_t>();
    m.shown_off = c->rr_off.as<uint32_t>();
    m.shown = c->rr_text.as<unsigned char>();
    m.n_shown = (uint32_t)c->rr_n;
    m.read_len = c->rm_len.as<unsigned long long>();
    m.flags = c->rr_flags.as<uint32_t>();
    m.n_reads = n_reads;
    m.unassigned = c->rr_unassigned;
    if (lists) {
        L.subj = c->cur_subj;
        L.qoff = c->cur_qoff;
        L.subj_feat = c->subj_feat.as<int32_t>();
        L.n_subjects = (uint32_t)std::max(c->n_subjects, 0);
        L.anc = anc;
        L.n_nodes = (uint32_t)std::max(c->n_nodes, 0);
        L.key_off = c->rl_n ? c->rl_off.as<uint32_t>() : m.shown_off;
        L.key = c->rl_n ? c->rl_text.as<unsigned char>() : m.shown;
        L.pairs = c->rl_pairs.as<uint2>();
        L.n_pairs = c->rl_npairs.as<uint32_t>();
    }
    const int32_t* samp = c->rd_samp.as<int32_t>();
    const dim3 rgrid((n_reads + kDtokThreads - 1) / kDtokThreads);
    HIP_TRY(c, hipMemsetAsync(c->rr_flags.p, 0, 16, c->stream));
    // (the family's bracket is closed on every way out)
    struct KtClose {
        wk_ctx* c;
        KernelTimer* t;
        void close() {
            if (t) ktimer_end(c, t);
            t = nullptr;
        }
        ~KtClose() { close(); }
    } kt{c, ktimer_begin(c, lists ? "readmap_lists_demux" : "readmap_reads_demux")};
    if (lists)
        hipLaunchKernelGGL(readmap_lists_build_demux_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, L, samp);
    else
        hipLaunchKernelGGL(readmap_reads_len_demux_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, m, samp);
    HIP_TRY(c, hipGetLastError());
    uint32_t flags = 0;
    HIP_TRY(c, hipMemcpyAsync(&flags, c->rr_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
    unsigned long long total = 0;
    const int rc = part_places(c, samp, m.read_len, n_reads, c->rd_cols, &total);
    if (rc) return rc;
    if (flags) {
        return fail(c, WK_E_STATE, "job %d left a code or a list that the tables cannot print (%d features shown, %d subjects)", job, c->rr_n,
                    c->n_subjects);
    }
    if (total >= (1ull << 40)) return fail(c, WK_E_RANGE, "read-map text of one block beyond 2^40 bytes");
    if (total > 0) {
        HIP_TRY(c, c->rm_text.reserve((size_t)total + 64));
        m.out = c->rm_text.as<unsigned char>();
        m.out_cap = total;
        m.read_len = c->pd_off.as<unsigned long long>();  // (the places the partition gave the lines)
        if (lists)
            hipLaunchKernelGGL(readmap_lists_write_demux_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, L, samp);
        else
            hipLaunchKernelGGL(readmap_reads_write_demux_kernel, rgrid, dim3(kDtokThreads), 0, c->stream, a, m, samp);
        HIP_TRY(c, hipGetLastError());
    }
    kt.close();
    c->rm_bytes = (int64_t)total;
    c->rd_segs = (int32_t)c->rd_cols;
    *n_bytes = (int64_t)total;
    *n_segments = c->rd_segs;
    return WK_OK;
}

int wk_dtok_readmap_reads_demux(wk_ctx* c, int32_t job, int64_t* n_bytes, int32_t* n_segments) {
    return readmap_demux_impl(c, job, n_bytes, n_segments, false);
}

int wk_dtok_readmap_lists_demux(wk_ctx* c, int32_t job, int64_t* n_bytes, int32_t* n_segments) {
    return readmap_demux_impl(c, job, n_bytes, n_segments, true);
}

int wk_dtok_readmap_segments(wk_ctx* c, uint64_t* seg, int32_t cap) {
    if (!c || cap < 0 || (cap > 0 && !seg)) return WK_E_ARG;
    if (cap < c->rd_segs) return fail(c, WK_E_CAPACITY, "need room for %d segments", c->rd_segs);
    if (c->rd_segs == 0) return WK_OK;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(seg, c->pd_seg.p, (size_t)c->rd_segs * 3 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// (tests) the partition alone on arrays of the caller's.  *status = 1: tiles x samples beyond the capacity -- nothing
// is written.
int wk_readmap_demux_partition(wk_ctx* c, const int32_t* samp, const uint64_t* len, int64_t n, uint64_t* off, uint64_t* seg, int32_t seg_cap,
                               int32_t* n_seg, uint64_t* total, int* status) {
    if (!c || n < 0 || n >= (1ll << 32) - 1 || (n > 0 && (!samp || !len || !off)) || seg_cap < 0 || (seg_cap > 0 && !seg) || !n_seg || !total || !status)
        return WK_E_ARG;
    *status = 1;
    DeviceGuard guard(c->device);
    // (the staged chunk's columns and places are overwritten)
    c->rd_chunk = false;
    c->rd_segs = 0;
    DevBuf d_samp, d_len;
    struct Free {
        DevBuf &a, &b;
        ~Free() {
            a.release();
            b.release();
        }
    } free_bufs{d_samp, d_len};
    HIP_TRY(c, d_samp.reserve((size_t)std::max<int64_t>(n, 1) * 4));
    HIP_TRY(c, d_len.reserve((size_t)std::max<int64_t>(n, 1) * 8));
    if (n > 0) {
        HIP_TRY(c, hipMemcpyAsync(d_samp.p, samp, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_len.p, len, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    uint32_t cols = 0;
    int rc = part_columns(c, d_samp.as<int32_t>(), (uint32_t)n, &cols);
    if (rc) return rc;
    const int64_t tiles = (n + kPartTile - 1) / kPartTile;
    if (tiles * (int64_t)cols > part_cap(c)) return WK_OK;
    if ((int64_t)cols > seg_cap) return fail(c, WK_E_CAPACITY, "need room for %u segments", cols);
    unsigned long long all = 0;
    if ((rc = part_places(c, d_samp.as<int32_t>(), d_len.as<unsigned long long>(), (uint32_t)n, cols, &all))) return rc;
    if (n > 0 && cols > 0) {
        HIP_TRY(c, hipMemcpyAsync(off, c->pd_off.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(seg, c->pd_seg.p, (size_t)cols * 3 * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
        for (int64_t r = 0; r < n; ++r) off[r] = 0;
    }
    *n_seg = (int32_t)cols;
    *total = all;
    *status = 0;
    return WK_OK;
}

static bool ordinal_tally_jobs(const wk_ctx* c, const wk_job* jobs, int32_t n_jobs) {
    bool tally = c->use_tally && !c->genes_by_index && c->slots > 0;
    for (int j = 0; j < n_jobs && tally; ++j)
        tally = jobs[j].mode == WK_MODE_NONE && !(jobs[j].flags & (WK_F_UNIQ | WK_F_SIZED));
    return tally;
}

// wk_dtok_stage_hits, the block's hits placed BEHIND those of the blocks staged this way since the last count:
// a 64 MB block of text brings 1.5 M hits, the sorted match (wk_stripe.hpp) pays from a few million on.
// *may_wait = 1: the caller may stage the next block before it counts (`jobs` are of the kind the sorted match
// serves, the pile is still below what it wants); 0: count now.  Whatever is piled up is one chunk for
// wk_ordinal_count / wk_ordinal_match, with one group for all of it (wk_set_uniform_group) unless a strata map
// on the device names the reads' groups.
int wk_dtok_stage_hits_append(wk_ctx* c, const int32_t* genome_of_subject, int32_t n_subjects, double th, const wk_job* jobs,
                              int32_t n_jobs, int64_t* n_reads, int64_t* n_hits, int* status, int* may_wait) {
    if (!c || !may_wait || n_jobs < 0 || (n_jobs > 0 && !jobs)) return WK_E_ARG;
    *may_wait = 0;
    const int rc = dtok_stage_impl(c, genome_of_subject, n_subjects, th, true, n_reads, n_hits, status);
    if (rc || *status != 0) return rc;
    *may_wait = n_jobs > 0 && n_jobs <= WK_MAX_JOBS && !c->s_use && ordinal_tally_jobs(c, jobs, n_jobs) && c->use_stripes &&
                        c->stripes_usable && c->stripes_host.size() <= kStripeMax && c->n_hits < c->stripes_min_hits
                    ? 1
                    : 0;
    return WK_OK;
}

// ---- ordinal -------------------------------------------------------------------

int wk_ordinal_stage(wk_ctx* c, const int32_t* genome, const int32_t* beg, const int32_t* end, const uint32_t* len,
                     int64_t n_hits, const int32_t* hoff, int64_t n_reads, const int32_t* group, double th) {
    if (!c) return WK_E_ARG;
    if (n_hits < 0 || n_reads < 0 || !hoff || (n_hits > 0 && (!genome || !beg || !end || !len)))
        return fail(c, WK_E_ARG, "bad ordinal chunk arguments");
    if (n_hits >= (1ll << 31)) return fail(c, WK_E_RANGE, "more than 2^31 hits in one chunk");
    if (hoff[0] != 0 || hoff[n_reads] != n_hits) return fail(c, WK_E_ARG, "hoff must run from 0 to n_hits");
    if (!(th > 0.0)) return fail(c, WK_E_ARG, "overlap threshold must be positive");
    if (c->acc_open) return fail(c, WK_E_STATE, "staged hits not counted yet (wk_ordinal_count)");
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = upload(c, c->o_genome, genome, (size_t)n_hits * 4))) return rc;
    if ((rc = upload(c, c->o_beg, beg, (size_t)n_hits * 4))) return rc;
    if ((rc = upload(c, c->o_end, end, (size_t)n_hits * 4))) return rc;
    if ((rc = upload(c, c->o_len, len, (size_t)n_hits * 4))) return rc;
    if ((rc = upload(c, c->o_hoff, hoff, ((size_t)n_reads + 1) * 4))) return rc;
    if (group && (rc = upload(c, c->c_group, group, (size_t)n_reads * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->n_hits = n_hits;
    c->o_reads = n_reads;
    c->th = th;
    c->has_group = group != nullptr;
    c->dx_hits = false;
    c->group_base = 0;
    c->rk_valid[0] = c->rk_valid[1] = false;
    c->ord_valid = true;
    c->sb_valid = false;
    c->chunk_valid = false;
    return WK_OK;
}

// Launch of match_hits_kernel: per-genome words in LDS when they fit.
// The dense log of the gene tally (wk_ordinal.hpp): genes go to the partition their low bits name, a partition is summed in
// an LDS array of 64-bit weights indexed by the high bits.  As few partitions as that array allows: every (workgroup,
// partition) stream has a line open in L2, and 768 x 256 of them (25 MB) did not stay there — the scattered 4-byte stores
// went out as partial lines, 1.08 GB written for 0.34 GB of entries (profiles/r03_ordinal_pmc_summary.txt).
static bool range_log_shape(const wk_ctx* c, uint32_t* parts, uint32_t* span) {
    constexpr uint32_t kSpanMax = 16384;  // 128 KiB of LDS
    uint32_t p = c->range_parts_opt > 0 ? (uint32_t)c->range_parts_opt : 16u;
    while (p < kLogPartsMax && (uint32_t)(c->max_gene_feature / (int32_t)p) + 1u > kSpanMax) p <<= 1;
    *parts = p;
    *span = (uint32_t)(c->max_gene_feature / (int32_t)p) + 1u;
    return *span <= kSpanMax && c->max_gene_feature < (1 << 28);
}

static int launch_match_hits(wk_ctx* c, bool counts) {
    MatchArgs a{};
    a.genome = c->o_genome.as<int32_t>();
    a.beg = c->o_beg.as<int32_t>();
    a.end = c->o_end.as<int32_t>();
    a.len = c->o_len.as<uint32_t>();
    a.n_hits = c->n_hits;
    a.th = c->th;
    a.gene4 = c->gene4.as<int4>();
    a.grid = c->g_grid.as<int32_t>();
    a.gfirst = c->g_first.as<int32_t>();
    a.goff = c->g_goff.as<int32_t>();
    a.gshift = c->g_shift.as<unsigned char>();
    a.n_genomes = c->n_genomes;
    a.ablate = c->ablate;
    const int64_t n_tiles = (c->n_hits + kMatchTile - 1) / kMatchTile;
    const int64_t rounds = (n_tiles + kMatchGroup - 1) / kMatchGroup;
    // 9 bytes per genome; three workgroups of 512 threads per CU while the
    // registers (80 without the counts) and the LDS copies allow
    const size_t info = ((size_t)c->n_genomes * 2 + 1) * 4 + (size_t)c->n_genomes + 16;
    const bool in_lds = c->match_lds && info <= (size_t)150 * 1024;
    const int by_regs = counts ? 2 : 3;
    const int per_cu = !in_lds ? by_regs : std::max(1, std::min(by_regs, (int)((size_t)156 * 1024 / info)));
    const dim3 grid((unsigned)std::min<int64_t>(rounds, (int64_t)c->prop.multiProcessorCount * per_cu));
    const dim3 block(kMatchThreads * kMatchGroup);
    int2* f2 = c->o_first2.as<int2>();
    int32_t* start = c->o_ub.as<int32_t>();
    int32_t* cnt = c->o_cnt.as<int32_t>();
    unsigned long long* ts = c->o_tile_sum.as<unsigned long long>();
    if (in_lds && counts)
        hipLaunchKernelGGL((match_hits_kernel<true, true>), grid, block, info, c->stream, a, f2, start, cnt, ts);
    else if (in_lds)
        hipLaunchKernelGGL((match_hits_kernel<true, false>), grid, block, info, c->stream, a, f2, start, cnt, ts);
    else if (counts)
        hipLaunchKernelGGL((match_hits_kernel<false, true>), grid, block, 0, c->stream, a, f2, start, cnt, ts);
    else
        hipLaunchKernelGGL((match_hits_kernel<false, false>), grid, block, 0, c->stream, a, f2, start, cnt, ts);
    HIP_TRY(c, hipGetLastError());
    return WK_OK;
}

// Gene lists per read from the matches (offset scan, lists, read offsets);
// `matched`: match_hits_kernel already ran with counts.
static int materialise_gene_lists(wk_ctx* c) {
    const int64_t n_hits = c->n_hits;
    const int64_t n_tiles = (n_hits + kMatchTile - 1) / kMatchTile;
    HIP_TRY(c, c->o_poff.reserve((size_t)(n_hits ? n_hits : 1) * 4));
    HIP_TRY(c, c->o_tile_off.reserve((size_t)(n_tiles ? n_tiles : 1) * 8));
    HIP_TRY(c, c->o_qoff.reserve(((size_t)c->o_reads + 1) * 4));
    unsigned long long total = 0;
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 3), 0, 8, c->stream));
    if (n_hits > 0) {
        KernelTimer* kt = ktimer_begin(c, "scan");
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->o_tile_sum.as<unsigned long long>(),
                           c->o_tile_off.as<unsigned long long>(), n_tiles, scalar_u64(c, 3));
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&total, scalar_u64(c, 3), 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (total >= (1ull << 31)) return fail(c, WK_E_RANGE, "more than 2^31 read-gene pairs in one chunk; stage fewer hits");
        HIP_TRY(c, c->o_pairs.reserve((size_t)(total ? total : 1) * 4));
        MatchArgs a{};
        a.beg = c->o_beg.as<int32_t>();
        a.end = c->o_end.as<int32_t>();
        a.len = c->o_len.as<uint32_t>();
        a.n_hits = n_hits;
        a.th = c->th;
        a.gene4 = c->gene4.as<int4>();
        kt = ktimer_begin(c, "match_write");
        hipLaunchKernelGGL(match_write_kernel, dim3((unsigned)n_tiles), dim3(kMatchThreads), 0, c->stream, a,
                           c->o_cnt.as<int32_t>(), c->o_ub.as<int32_t>(), c->o_first2.as<int2>(), c->o_tile_off.as<unsigned long long>(), c->o_poff.as<int32_t>(),
                           c->o_pairs.as<int32_t>());
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
    } else {
        HIP_TRY(c, c->o_pairs.reserve(4));
    }
    hipLaunchKernelGGL(read_offsets_kernel, dim3((unsigned)((c->o_reads + 1 + 255) / 256)), dim3(256), 0, c->stream,
                       c->o_hoff.as<int32_t>(), c->o_poff.as<int32_t>(), c->o_reads, n_hits, scalar_u64(c, 3),
                       c->o_qoff.as<int32_t>());
    HIP_TRY(c, hipGetLastError());
    c->stat_pairs += (int64_t)total;
    // the per-read gene lists become the current classify chunk
    c->cur_subj = c->o_pairs.as<int32_t>();
    if (c->genes_by_index) {  // (the lists name genes by table index: their features for the classification)
        HIP_TRY(c, c->o_pairs_feat.reserve((size_t)(total ? total : 1) * 4));
        if (total > 0) {
            hipLaunchKernelGGL(gather_i32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                               c->o_pairs.as<int32_t>(), c->g_feature.as<int32_t>(), (int64_t)total, (int64_t)c->n_genes,
                               c->o_pairs_feat.as<int32_t>());
            HIP_TRY(c, hipGetLastError());
        }
        c->cur_subj = c->o_pairs_feat.as<int32_t>();
    }
    c->cur_qoff = c->o_qoff.as<int32_t>();
    c->n_reads = c->o_reads;
    c->n_records = (int64_t)total;
    c->subj_is_set = false;  // several hits of a read may match the same gene
    c->subj_indexed = false; // gene lists carry feature ids
    c->chunk_valid = true;
    c->dx_chunk = false;
    c->rr_chunk = false;
    c->rd_chunk = false;
    return WK_OK;
}

static int reserve_match_buffers(wk_ctx* c) {
    const int64_t n_hits = c->n_hits;
    const int64_t n_tiles = (n_hits + kMatchTile - 1) / kMatchTile;
    HIP_TRY(c, c->o_cnt.reserve((size_t)(n_hits ? n_hits : 1) * 4));
    HIP_TRY(c, c->o_ub.reserve((size_t)(n_hits ? n_hits : 1) * 4));
    HIP_TRY(c, c->o_first2.reserve((size_t)(n_hits ? n_hits : 1) * 8));
    HIP_TRY(c, c->o_tile_sum.reserve((size_t)(n_tiles ? n_tiles : 1) * 8));
    return WK_OK;
}

int wk_ordinal_match(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    if (!c->ord_valid) return fail(c, WK_E_STATE, "no ordinal chunk staged");
    if (!c->genes_set) return fail(c, WK_E_STATE, "no gene tables uploaded (wk_set_genes)");
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    c->acc_open = false;
    int rc = reserve_match_buffers(c);
    if (rc) return rc;
    if (c->n_hits > 0) {
        KernelTimer* kt = ktimer_begin(c, "match_count");
        if ((rc = launch_match_hits(c, true))) return rc;
        ktimer_end(c, kt);
    }
    if ((rc = materialise_gene_lists(c))) return rc;
    if (c->dx_hits && c->o_reads > 0) {  // (the samples whose reads matched a gene: in front of whatever classifies or fetches the chunk)
        hipLaunchKernelGGL(demux_met_hits_kernel, dim3((unsigned)((c->o_reads + kDtokThreads - 1) / kDtokThreads)), dim3(kDtokThreads), 0,
                           c->stream, c->o_qoff.as<int32_t>(), c->c_group.as<int32_t>(), c->dx_rsamp.as<int32_t>(), c->o_reads,
                           (uint32_t)c->dx_name_off_host.size(), c->dx_met.as<unsigned char>());
        HIP_TRY(c, hipGetLastError());
    }
    return WK_OK;
}

int wk_ordinal_hit_offsets(wk_ctx* c, int32_t* poff, int64_t cap) {
    if (!c || !poff) return WK_E_ARG;
    if (!c->chunk_valid || (c->cur_subj != c->o_pairs.as<int32_t>() && c->cur_subj != c->o_pairs_feat.as<int32_t>()))
        return fail(c, WK_E_STATE, "no gene lists staged (wk_ordinal_match)");
    if (cap < c->n_hits + 1) return fail(c, WK_E_CAPACITY, "need %lld offsets", (long long)c->n_hits + 1);
    DeviceGuard guard(c->device);
    if (c->n_hits) HIP_TRY(c, hipMemcpyAsync(poff, c->o_poff.p, (size_t)c->n_hits * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    poff[c->n_hits] = (int32_t)c->n_records;
    return WK_OK;
}

int wk_ordinal_pair_genes(wk_ctx* c, int32_t* out, int64_t cap) {
    if (!c || (cap > 0 && !out)) return WK_E_ARG;
    if (!c->genes_by_index) return fail(c, WK_E_STATE, "the gene lists carry features (option gene_index_pairs before wk_set_genes)");
    if (!c->chunk_valid || c->cur_subj != c->o_pairs_feat.as<int32_t>()) return fail(c, WK_E_STATE, "no gene lists staged (wk_ordinal_match)");
    if (cap < c->n_records) return fail(c, WK_E_CAPACITY, "need %lld entries", (long long)c->n_records);
    DeviceGuard guard(c->device);
    if (c->n_records) HIP_TRY(c, hipMemcpyAsync(out, c->o_pairs.p, (size_t)c->n_records * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

int wk_set_uniform_group(wk_ctx* c, int32_t group) {
    if (!c) return WK_E_ARG;
    if (group < 0 || group >= (1 << WK_KEY_GROUP_BITS)) return fail(c, WK_E_ARG, "group id outside [0, %d)", 1 << WK_KEY_GROUP_BITS);
    c->has_group = false;
    c->group_base = group;
    return WK_OK;
}

// The genes of the staged chunk's reads counted straight from the matches (rank none, one group): the
// gather kernels of wk_ordinal.hpp over c->o_* (match_hits -> first2 -> ordinal_tally -> log -> merge).
static int tally_count(wk_ctx* c, const wk_job* jobs, int32_t n_jobs) {
    int rc = reserve_match_buffers(c);
    if (rc) return rc;
    // (without the per-hit counts: they are only needed for reads the tally
    // leaves over, and then the matching runs once more)
    KernelTimer* kt = ktimer_begin(c, "match_count");
    if ((rc = launch_match_hits(c, false))) return rc;
    ktimer_end(c, kt);
    const int blocks = std::min(kStatBlocks, c->prop.multiProcessorCount * c->tally_per_cu);
    const int64_t n_words = (c->o_reads + 63) / 64;
    TallyArgs t{};
    t.hoff = c->o_hoff.as<int32_t>();
    t.first2 = c->o_first2.as<int2>();
    t.n_reads = c->o_reads;
    t.n_jobs = n_jobs;
    for (int j = 0; j < n_jobs; ++j) t.job_index[j] = j;
    t.group = c->group_base;
    t.table = CountTable{c->tkeys.as<unsigned long long>(), c->tvals.as<unsigned long long>(), c->slots - 1, scalar_err(c)};
    // one job over gene ids with at most 4096 per partition: the dense log (wk_ordinal.hpp)
    uint32_t range_parts = 0, range_span = 0;
    const bool by_range = range_log_shape(c, &range_parts, &range_span) && c->use_range_log && n_jobs == 1;
    // distinct keys: the genes (256 merge tables of 8192 slots hold ~1.3 M at a comfortable load)
    if (by_range)
        t.log_parts = range_parts;
    else
        t.log_parts = c->log_parts_opt ? (uint32_t)c->log_parts_opt : ((int64_t)c->n_genes * n_jobs <= 256 * 5120 ? 256u : kLogPartsMax);
    const int64_t streams = (int64_t)blocks * t.log_parts;
    const size_t entry = by_range ? 4 : 8;
    // every gene of a hit is one entry: hits with a gene rarely have two
    int64_t cap = 3 * (c->n_hits * (int64_t)n_jobs / streams + 1) + 16;
    cap = std::max<int64_t>(16, std::min<int64_t>(cap, c->plog_max_bytes / (int64_t)entry / streams));
    t.plog_cap = (uint32_t)cap;
    HIP_TRY(c, c->plog.reserve((size_t)streams * t.plog_cap * entry));
    HIP_TRY(c, c->plog_cnt.reserve((size_t)streams * 4));
    HIP_TRY(c, c->left_mask.reserve((size_t)n_words * 8));
    t.plog = c->plog.as<unsigned long long>();
    t.plog32 = c->plog.as<uint32_t>();
    t.plog_cnt = c->plog_cnt.as<uint32_t>();
    t.stat_block = c->stat_block.as<unsigned long long>();
    t.left_mask = c->left_mask.as<unsigned long long>();
    t.n_left = scalar_u64(c, 7);
    HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 7), 0, 16, c->stream));
    kt = ktimer_begin(c, "classify");
    if (by_range) {
        // LDS per workgroup: log cursors + 12 KiB queue + 16 KiB of gene sets
        const size_t tally_lds = (size_t)t.log_parts * 4 + (size_t)kTallyQueue * 4 + (size_t)kTallySlots * kTallyThreads * 4;
        hipLaunchKernelGGL(ordinal_tally_kernel<true>, dim3(blocks), dim3(kTallyThreads), tally_lds, c->stream, t, 0u);
        ktimer_end(c, kt);
        kt = ktimer_begin(c, "partition_merge");
        hipLaunchKernelGGL(range_merge_kernel, dim3(t.log_parts, kRangeMergeSplit), dim3(1024), (size_t)8 * range_span, c->stream, t.plog32,
                           t.plog_cnt, (uint32_t)blocks, t.plog_cap, range_span, 0u, (uint32_t)t.group, t.table);
        ktimer_end(c, kt);
    } else {
        // LDS per workgroup (three per CU): 16 KiB hash cache + log cursors + 12 KiB queue + 16 KiB of gene sets
        const uint32_t tally_slots = (uint32_t)std::max(256, std::min(c->tally_slots, 4096));
        const size_t tally_lds = (size_t)tally_slots * 16 + (size_t)t.log_parts * 4 + (size_t)kTallyQueue * 4 + (size_t)kTallySlots * kTallyThreads * 4;
        hipLaunchKernelGGL(ordinal_tally_kernel<false>, dim3(blocks), dim3(kTallyThreads), tally_lds, c->stream, t, tally_slots);
        ktimer_end(c, kt);
        kt = ktimer_begin(c, "partition_merge");
        hipLaunchKernelGGL(partition_merge_kernel, dim3(t.log_parts), dim3(1024), (size_t)8192 * 16, c->stream,
                           c->plog.as<unsigned long long>(), c->plog_cnt.as<uint32_t>(), (uint32_t)blocks, t.plog_cap, 8192u, t.table);
        ktimer_end(c, kt);
    }
    HIP_TRY(c, hipGetLastError());
    unsigned long long left_pairs[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(left_pairs, scalar_u64(c, 7), 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->chunk_valid = false;
    if (left_pairs[0] == 0) {
        c->stat_pairs += (int64_t)left_pairs[1];
        return WK_OK;
    }
    // reads the tally left out (many genes per hit / per read): their gene
    // lists through the generic evaluator
    if ((rc = launch_match_hits(c, true))) return rc;
    if ((rc = materialise_gene_lists(c))) return rc;
    c->listed_only = true;
    rc = wk_classify_staged(c, jobs, n_jobs, nullptr);
    c->listed_only = false;
    return rc;
}


// ---- the sorted coord-match (wk_stripe.hpp) ------------------------------------------------------
static StripeSortArgs stripe_sort_args(wk_ctx* c, uint32_t n_tiles) {
    StripeSortArgs a{};
    a.genome = c->o_genome.as<int32_t>();
    a.beg = c->o_beg.as<int32_t>();
    a.end = c->o_end.as<int32_t>();
    a.len = c->o_len.as<uint32_t>();
    a.hoff = c->o_hoff.as<int32_t>();
    a.n_reads = c->o_reads;
    a.stripe_of = c->g_stripe_of.as<int32_t>();
    a.n_genomes = c->n_genomes;
    a.n_stripes = (uint32_t)c->stripes_host.size();
    a.n_tiles = n_tiles;
    a.cnt = c->sb_cnt.as<uint32_t>();
    a.row_base = c->sb_base.as<unsigned long long>();
    a.binned = c->sb_binned.as<int4>();
    a.r_genome = c->r_genome.as<int32_t>();
    a.r_beg = c->r_beg.as<int32_t>();
    a.r_end = c->r_end.as<int32_t>();
    a.r_len = c->r_len.as<uint32_t>();
    a.r_hoff = c->r_hoff.as<int32_t>();
    return a;
}

// The staged chunk sorted: reads of one hit by genome stripe, the others compacted (once per staged chunk).
static int stripe_sort(wk_ctx* c) {
    if (c->sb_valid) return WK_OK;
    const uint32_t n_stripes = (uint32_t)c->stripes_host.size();
    const uint32_t n_tiles = (uint32_t)((c->o_reads + kStripeTileReads - 1) / kStripeTileReads);
    const size_t rows = (size_t)n_stripes + 2;
    HIP_TRY(c, c->sb_cnt.reserve(rows * n_tiles * 4));
    HIP_TRY(c, c->sb_tot.reserve(rows * 8));
    HIP_TRY(c, c->sb_base.reserve(rows * 8));
    // (every read could have one hit, or none: both outputs sized for the chunk)
    HIP_TRY(c, c->sb_binned.reserve((size_t)std::max<int64_t>(c->o_reads, 1) * 16));
    HIP_TRY(c, c->r_genome.reserve((size_t)std::max<int64_t>(c->n_hits, 1) * 4));
    HIP_TRY(c, c->r_beg.reserve((size_t)std::max<int64_t>(c->n_hits, 1) * 4));
    HIP_TRY(c, c->r_end.reserve((size_t)std::max<int64_t>(c->n_hits, 1) * 4));
    HIP_TRY(c, c->r_len.reserve((size_t)std::max<int64_t>(c->n_hits, 1) * 4));
    HIP_TRY(c, c->r_hoff.reserve(((size_t)c->o_reads + 1) * 4));
    const StripeSortArgs a = stripe_sort_args(c, n_tiles);
    KernelTimer* kt = ktimer_begin(c, "stripe_sort");
    hipLaunchKernelGGL(stripe_count_kernel, dim3(n_tiles), dim3(kStripeTileThreads), 0, c->stream, a);
    hipLaunchKernelGGL(stripe_rows_kernel, dim3((unsigned)rows), dim3(1024), 0, c->stream, c->sb_cnt.as<uint32_t>(), n_tiles,
                       c->sb_tot.as<unsigned long long>());
    hipLaunchKernelGGL(stripe_bases_kernel, dim3(1), dim3(64), 0, c->stream, c->sb_tot.as<unsigned long long>(),
                       c->sb_base.as<unsigned long long>(), n_stripes);
    hipLaunchKernelGGL(stripe_scatter_kernel, dim3(n_tiles), dim3(kStripeTileThreads), 0, c->stream, a);
    ktimer_end(c, kt);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned long long> tot(rows);
    HIP_TRY(c, hipMemcpyAsync(tot.data(), c->sb_tot.p, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the pieces of the stripes' hits, one workgroup each
    std::vector<StripeUnit> units;
    unsigned long long first = 0;
    for (uint32_t s = 0; s < n_stripes; ++s) {
        for (unsigned long long at = 0; at < tot[s]; at += kStripePiece)
            units.push_back(StripeUnit{s, (uint32_t)(first + at), (uint32_t)std::min<unsigned long long>(kStripePiece, tot[s] - at), 0u});
        first += tot[s];
    }
    c->sb_single = (int64_t)first;
    c->sb_rest_reads = (int64_t)tot[n_stripes];
    c->sb_rest_hits = (int64_t)tot[n_stripes + 1];
    c->sb_n_units = (uint32_t)units.size();
    if (!units.empty()) {
        int rc = upload(c, c->sb_units, units.data(), units.size() * sizeof(StripeUnit));
        if (rc) return rc;
    }
    const int32_t end = (int32_t)c->sb_rest_hits;  // r_hoff's last entry
    HIP_TRY(c, hipMemcpyAsync(c->r_hoff.as<int32_t>() + c->sb_rest_reads, &end, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sb_valid = true;
    return WK_OK;
}

static int stripe_count(wk_ctx* c, const wk_job* jobs, int32_t n_jobs) {
    int rc = stripe_sort(c);
    if (rc) return rc;
    HIP_TRY(c, c->sb_stat.reserve(64));
    HIP_TRY(c, hipMemsetAsync(c->sb_stat.p, 0, 64, c->stream));
    StripeMatchArgs m{};
    m.binned = c->sb_binned.as<int4>();
    m.units = c->sb_units.as<StripeUnit>();
    m.gene4 = c->gene4.as<int4>();
    m.gene_off = c->g_gene_off.as<int32_t>();
    m.stripes = c->g_stripes.as<StripeInfo>();
    m.grid = c->g_grid.as<int32_t>();
    m.gfirst = c->g_first.as<int32_t>();
    m.goff = c->g_goff.as<int32_t>();
    m.gshift = c->g_shift.as<unsigned char>();
    m.th = c->th;
    m.n_jobs = n_jobs;
    for (int j = 0; j < n_jobs; ++j) m.job_index[j] = j;
    m.group = c->group_base;
    m.table = CountTable{c->tkeys.as<unsigned long long>(), c->tvals.as<unsigned long long>(), c->slots - 1, scalar_err(c)};
    const uint32_t over_cap = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->sb_single, 1), 1 << 24);
    HIP_TRY(c, c->sb_over.reserve((size_t)over_cap * 4));
    m.overflow = c->sb_over.as<uint32_t>();
    m.overflow_cap = over_cap;
    m.stat = c->sb_stat.as<unsigned long long>();
    m.stat_block = c->stat_block.as<unsigned long long>();
    if (c->sb_n_units) {
        KernelTimer* kt = ktimer_begin(c, "stripe_match");
        hipLaunchKernelGGL(stripe_match_kernel, dim3(c->sb_n_units), dim3(kStripeMatchThreads), kStripeMatchLds, c->stream, m);
        ktimer_end(c, kt);
        HIP_TRY(c, hipGetLastError());
    }
    unsigned long long stat[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(stat, c->sb_stat.p, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stat[2] > over_cap) return fail(c, WK_E_CAPACITY, "more than %u hits with three or more genes in one chunk", over_cap);
    if (stat[2]) {
        hipLaunchKernelGGL(stripe_overflow_kernel, dim3((unsigned)stat[2]), dim3(64), 0, c->stream, m, (uint32_t)stat[2]);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(stat, c->sb_stat.p, 24, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->stat_pairs += (int64_t)stat[1];
    c->chunk_valid = false;
    if (c->sb_rest_reads == 0) return WK_OK;
    // the reads of several hits (and hits on genomes without a stripe): the gather kernels, over their own arrays
    auto swap_rest = [&]() {
        std::swap(c->o_genome, c->r_genome);
        std::swap(c->o_beg, c->r_beg);
        std::swap(c->o_end, c->r_end);
        std::swap(c->o_len, c->r_len);
        std::swap(c->o_hoff, c->r_hoff);
        std::swap(c->n_hits, c->sb_rest_hits);
        std::swap(c->o_reads, c->sb_rest_reads);
    };
    swap_rest();
    rc = tally_count(c, jobs, n_jobs);
    swap_rest();
    return rc;
}

int wk_ordinal_count(wk_ctx* c, const wk_job* jobs, int32_t n_jobs) {
    if (!c) return WK_E_ARG;
    if (!c->ord_valid) return fail(c, WK_E_STATE, "no ordinal chunk staged");
    if (!c->genes_set) return fail(c, WK_E_STATE, "no gene tables uploaded (wk_set_genes)");
    if (n_jobs < 1 || n_jobs > WK_MAX_JOBS || !jobs) return fail(c, WK_E_ARG, "n_jobs must be in [1, %d]", WK_MAX_JOBS);
    // the genes themselves are counted (rank none, one group, no size
    // normalisation): tallied per read straight from the matches
    const bool tally = ordinal_tally_jobs(c, jobs, n_jobs) && !c->has_group && c->n_hits > 0 && c->o_reads > 0;
    c->acc_open = false;   // (whatever was piled up is counted by this call)
    if (!tally) {
        int rc = wk_ordinal_match(c);
        if (rc) return rc;
        return wk_classify_staged(c, jobs, n_jobs, nullptr);
    }
    DeviceGuard guard(c->device);
    KtScope kt_scope(c);
    // The sorted match pays for chunks that are large against its fixed costs (a scan over stripes x tiles, a
    // unit per stripe that loads the stripe's genes into LDS, one more read-back): from a few million hits on.
    // The text route stages a block's hits at a time (~1.6 M): those keep the gather kernels, at 80 us per
    // block against 370 (profiles/r05_e2e_ordinal_kernel_stats.csv).
    if (c->use_stripes && c->stripes_usable && c->stripes_host.size() <= kStripeMax && c->n_hits >= c->stripes_min_hits) {
        ++c->chunks_sorted;
        return stripe_count(c, jobs, n_jobs);
    }
    ++c->chunks_gathered;
    return tally_count(c, jobs, n_jobs);
}

int wk_chunk_download(wk_ctx* c, int32_t* subj, int64_t subj_cap, int32_t* qoff, int64_t qoff_cap, int64_t* n_records,
                      int64_t* n_reads) {
    if (!c) return WK_E_ARG;
    if (!c->chunk_valid) return fail(c, WK_E_STATE, "no chunk staged");
    if (n_records) *n_records = c->n_records;
    if (n_reads) *n_reads = c->n_reads;
    if (!subj && !qoff) return WK_OK;
    if ((subj && subj_cap < c->n_records) || (qoff && qoff_cap < c->n_reads + 1)) return fail(c, WK_E_CAPACITY, "download buffers too small");
    DeviceGuard guard(c->device);
    if (subj && c->n_records) HIP_TRY(c, hipMemcpyAsync(subj, c->cur_subj, (size_t)c->n_records * 4, hipMemcpyDeviceToHost, c->stream));
    if (qoff) HIP_TRY(c, hipMemcpyAsync(qoff, c->cur_qoff, ((size_t)c->n_reads + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WK_OK;
}

// ---- statistics & timing -------------------------------------------------------

int wk_get_stats(wk_ctx* c, wk_stats* out) {
    if (!c || !out) return WK_E_ARG;
    DeviceGuard guard(c->device);
    std::vector<unsigned long long> part((size_t)kStatBlocks * 2);
    HIP_TRY(c, hipMemcpyAsync(part.data(), c->stat_block.p, part.size() * 8, hipMemcpyDeviceToHost, c->stream));
    unsigned long long used = 0;
    if (c->slots) {
        HIP_TRY(c, hipMemsetAsync(scalar_u64(c, 4), 0, 8, c->stream));
        hipLaunchKernelGGL(table_count_kernel, dim3(grid_for((int64_t)c->slots, 256, 2048)), dim3(256), 0, c->stream,
                           c->tkeys.as<unsigned long long>(), c->slots, scalar_u64(c, 4));
        HIP_TRY(c, hipMemcpyAsync(&used, scalar_u64(c, 4), 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long s[2] = {0, 0};
    for (int b = 0; b < kStatBlocks; ++b) {
        s[0] += part[2 * b];
        s[1] += part[2 * b + 1];
    }
    out->n_reads = (int64_t)s[0] + c->stat_extra_reads + (c->w_open ? c->w_reads : 0);
    out->n_records = (int64_t)s[1] + c->stat_extra_records + (c->w_open ? c->w_records : 0);
    out->n_pairs = c->stat_pairs;
    out->table_used = (int64_t)used;
    return WK_OK;
}

int wk_reset_stats(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipMemsetAsync(c->stat_block.p, 0, (size_t)kStatBlocks * 16, c->stream));
    c->stat_pairs = 0;
    c->stat_extra_reads = c->stat_extra_records = 0;
    return WK_OK;
}

int wk_timer_begin(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    c->timer_closed = false;
    HIP_TRY(c, hipEventRecord(c->t0, c->stream));
    return WK_OK;
}

int wk_timer_end(wk_ctx* c) {
    if (!c) return WK_E_ARG;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipEventRecord(c->t1, c->stream));
    c->timer_closed = true;
    return WK_OK;
}

int wk_timer_ms(wk_ctx* c, double* ms) {
    if (!c || !ms) return WK_E_ARG;
    if (!c->timer_closed) return fail(c, WK_E_STATE, "timer region not closed");
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipEventSynchronize(c->t1));
    float f = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&f, c->t0, c->t1));
    *ms = (double)f;
    return WK_OK;
}

int wk_profile_kernels(wk_ctx* c, int enable) {
    if (!c) return WK_E_ARG;
    c->profile = enable != 0;
    return WK_OK;
}

int wk_last_kernel_ms(wk_ctx* c, const char* family, double* ms) {
    if (!c || !family || !ms) return WK_E_ARG;
    auto it = c->ktimers.find(family);
    if (it == c->ktimers.end() || !it->second.valid) return fail(c, WK_E_STATE, "no timed launch of kernel family '%s'", family);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipEventSynchronize(it->second.b));
    float f = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&f, it->second.from, it->second.b));
    *ms = (double)f;
    return WK_OK;
}

}  // extern "C"
