// wk_dinflate.hpp — gzip members that state their size, inflated on the device: one wave per member.
//
// The host has walked the chain (BGZF 'BC' / this package's 'WK' subfield: wk_inflate.cpp) and knows of every member
// where its DEFLATE stream begins (lo), where the member ends (hi; the trailer is the eight bytes before) and where
// its text goes (off: running sum of ISIZE).  The members are independent streams, so a wave takes one, decodes it
// with wk_dinflate_core.hpp -- the same functions the host test runs under AddressSanitizer -- and takes the next
// from a counter, until none is left: a launch with more members than resident waves balances itself.
//
// What the wave adds to the core is storage (DevIo):
//  * the last 34 KB of the member's output live in LDS as a ring (a match reaches back 32 KB at most); symbol decode
//    is uniform over the wave (every value the core sees comes through readfirstlane, so its state lives in scalar
//    registers), literals are stored by one lane, matches and stored bytes are copied by all 64;
//  * whenever 2 KB are complete they leave for HBM as 512 dwords, 8 per lane, and every lane folds its 32 bytes
//    into a CRC state of its own (CrcLanes); the states are joined when the member ends, so the member's CRC-32 is
//    verified here and the text never goes back to the host for it;
//  * compressed bytes come through a 1 KB stage in LDS, filled by byte loads that are masked to [lo, hi - 8);
//  * the block's tables (3.7 KB) are written by lane 0 and read through readfirstlane -- lane 0's own load, which
//    follows its stores in program order.
// 39 KB of LDS per wave: four workgroups of one wave per CU, one per SIMD.  HBM is written only by the 2 KB runs and
// the tail, all of them inside [off[i], off[i + 1]) by the core's bounds; nothing is read back from it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wk_dinflate_core.hpp"

namespace wk {

constexpr uint32_t kDinfRing = 17 * dinf::kFlush;   // 34 816: the window, a symbol's 258 bytes, and a run not yet gone
constexpr uint32_t kDinfStage = 1024;
constexpr int kDinfWavesPerCu = 4;

struct DinfIo {
    const unsigned char* in;    // blob + lo
    const unsigned char* tr;    // blob + hi - 8
    unsigned char* out;         // text + off[i]
    unsigned char* ring;
    uint32_t* stage;
    uint32_t n_in;
    uint32_t lane;
    uint32_t sbase, sn;         // the stage holds compressed bytes [sbase, sbase + sn)
    uint32_t crc_s, xgap, xrest, crc_t;

    __device__ __forceinline__ static uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }   // (one wave per workgroup: a fence for LDS, no waiting)

    __device__ __forceinline__ uint32_t ld16(const uint16_t* p) const { return uni(*p); }
    __device__ __forceinline__ uint32_t ld8(const uint8_t* p) const { return uni(*p); }
    __device__ __forceinline__ void st16(uint16_t* p, uint32_t v) const {
        if (lane == 0) *p = (uint16_t)v;
    }
    __device__ __forceinline__ void st8(uint8_t* p, uint32_t v) const {
        if (lane == 0) *p = (uint8_t)v;
    }
    // (lane 0 as well: what it reads back must be its own stores)
    __device__ __forceinline__ void fill16(uint16_t* p, uint32_t n) const {
        if (lane == 0)
            for (uint32_t i = 0; i < n / 2; ++i) reinterpret_cast<uint32_t*>(p)[i] = 0;
    }
    __device__ __forceinline__ void spread16(uint16_t* p, uint32_t start, uint32_t step, uint32_t end, uint32_t v) const {
        if (lane == 0)
            for (uint32_t i = start; i < end; i += step) p[i] = (uint16_t)v;
    }

    __device__ __forceinline__ void restage(uint32_t ip) {
        sync();
        sbase = ip;
        sn = n_in - ip < kDinfStage ? n_in - ip : kDinfStage;
        for (uint32_t w = lane; w < kDinfStage / 4; w += 64) {
            uint32_t v = 0;
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t b = 4 * w + j;
                if (b < sn) v |= (uint32_t)in[sbase + b] << (8 * j);
            }
            stage[w] = v;
        }
        sync();
    }
    __device__ __forceinline__ uint32_t in32(uint32_t ip) {
        if (ip < sbase || ip + 4 > sbase + sn || ((ip - sbase) & 3u)) restage(ip);
        return uni(stage[(ip - sbase) >> 2]);
    }
    __device__ __forceinline__ uint32_t in8(uint32_t ip) {
        if (ip < sbase || ip >= sbase + sn) restage(ip);
        return (uni(stage[(ip - sbase) >> 2]) >> (8 * ((ip - sbase) & 3u))) & 0xFFu;
    }
    __device__ __forceinline__ uint32_t trailer32(uint32_t k) const {
        uint32_t v = 0;
        for (uint32_t j = 0; j < 4; ++j) v |= (uint32_t)tr[4 * k + j] << (8 * j);
        return uni(v);
    }

    __device__ __forceinline__ void put(uint32_t p, uint32_t b) const {
        if (lane == 0) ring[p % kDinfRing] = (unsigned char)b;
    }
    // n <= 258 bytes from `src` to `dst`, src + n <= dst: every byte read was written before this call
    __device__ __forceinline__ void copy(uint32_t dst, uint32_t src, uint32_t n) const {
        sync();
        const uint32_t d0 = dst % kDinfRing, s0 = src % kDinfRing;
        for (uint32_t i = lane; i < n; i += 64) {
            uint32_t s = s0 + i, d = d0 + i;
            s = s >= kDinfRing ? s - kDinfRing : s;
            d = d >= kDinfRing ? d - kDinfRing : d;
            ring[d] = ring[s];
        }
    }
    // n <= 256 bytes of a stored block
    __device__ __forceinline__ void copy_in(uint32_t dst, uint32_t ip, uint32_t n) const {
        const uint32_t d0 = dst % kDinfRing;
        for (uint32_t i = lane; i < n; i += 64) {
            uint32_t d = d0 + i;
            d = d >= kDinfRing ? d - kDinfRing : d;
            ring[d] = in[ip + i];
        }
    }
    // output [p, p + kFlush) is complete (p a multiple of kFlush, so the run does not wrap in the ring)
    __device__ __forceinline__ void flush(uint32_t p) {
        sync();
        const uint32_t* rw = reinterpret_cast<const uint32_t*>(ring + p % kDinfRing);
        for (uint32_t j = 0; j < dinf::kFlush / 256; ++j) {
            const uint32_t w = j * 64 + lane, v = rw[w];
            __builtin_memcpy(out + p + 4 * w, &v, 4);
        }
        uint32_t mine[dinf::kPiece / 4];
        for (uint32_t j = 0; j < dinf::kPiece / 4; ++j) mine[j] = rw[lane * (dinf::kPiece / 4) + j];
        crc_s = dinf::CrcLanes::run(crc_s, xgap, mine);
    }
    __device__ __forceinline__ void flush_tail(uint32_t p, uint32_t n) {
        sync();
        const unsigned char* r = ring + p % kDinfRing;
        for (uint32_t i = lane; i < n; i += 64) out[p + i] = r[i];
        const uint32_t m = dinf::CrcLanes::tail_bytes(lane, n);
        uint32_t t = 0;
        for (uint32_t k = 0; k < m; ++k) t = dinf::crc_byte(t, r[lane * dinf::kPiece + k]);
        crc_t = t;
    }
    __device__ __forceinline__ uint32_t crc0(uint32_t n_tail) const {
        uint32_t r = dinf::CrcLanes::last(crc_s, lane, xrest, n_tail, crc_t, dinf::CrcLanes::tail_bytes(lane, n_tail));
        for (int d = 32; d >= 1; d >>= 1) r ^= __shfl_xor(r, d, 64);
        return uni(r);
    }
};

// status[i] = dinf::Status of member i; *any |= 1 if one failed.  *counter is 0 at the launch.
__global__ __launch_bounds__(64) void dinflate_kernel(const unsigned char* __restrict__ blob, const int64_t* __restrict__ lo,
                                                      const int64_t* __restrict__ hi, const int64_t* __restrict__ off, uint32_t n_members,
                                                      unsigned char* out, uint32_t* __restrict__ status, uint32_t* any,
                                                      uint32_t* counter) {
    __shared__ __align__(16) unsigned char ring[kDinfRing];
    __shared__ __align__(16) uint32_t stage[kDinfStage / 4];
    __shared__ dinf::Tables tables;
    const uint32_t lane = threadIdx.x;
    const uint32_t xgap = dinf::CrcLanes::gap(), xrest = dinf::CrcLanes::rest(lane);
    for (;;) {
        uint32_t m = 0;
        if (lane == 0) m = atomicAdd(counter, 1u);
        m = DinfIo::uni(m);
        if (m >= n_members) break;
        const int64_t l = lo[m], h = hi[m], o0 = off[m], o1 = off[m + 1];
        uint32_t st = dinf::kBadSpans;
        if (l >= 0 && h - l >= 8 && h - l < (1ll << 31) && o0 >= 0 && o1 >= o0 && o1 - o0 < (1ll << 31)) {
            DinfIo io;
            io.in = blob + l;
            io.tr = blob + h - 8;
            io.out = out + o0;
            io.ring = ring;
            io.stage = stage;
            io.n_in = (uint32_t)(h - l - 8);
            io.lane = lane;
            io.sbase = io.sn = 0;
            io.crc_s = io.crc_t = 0;
            io.xgap = xgap;
            io.xrest = xrest;
            dinf::Inflater<DinfIo> inf(io, &tables, io.n_in, (uint32_t)(o1 - o0));
            st = DinfIo::uni((uint32_t)inf.run());
        }
        if (lane == 0) {
            status[m] = st;
            if (st) atomicOr(any, 1u);
        }
        __syncthreads();
    }
}

}  // namespace wk
