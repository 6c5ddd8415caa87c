// wk_dinflate_core.hpp — one gzip member's DEFLATE stream inflated inside its own spans (wk_dinflate.hpp).
//
// Everything that decides bytes, as plain functions that are the same on the host and on the device: the bit reader,
// the code lengths of a dynamic block and their canonical tables, stored / fixed / dynamic blocks, the length and
// distance tables, the rule for matches that overlap their own output, and CRC-32 in pieces.  Storage is left to an
// `Io` the caller hands in: where the compressed bytes come from, where a byte of output goes, how a copy inside
// the output is carried out and what a finished run of output is folded into.  The kernel's Io keeps the last 32 KB
// in LDS and lets 64 lanes copy; tests/native/dinflate_core_host.cpp has one over two plain arrays of exactly the
// sizes stated, under AddressSanitizer.  The Io is never asked for anything outside the member's spans:
//
//  * compressed bytes: in8(i) with i < n_in and in32(i) with i + 4 <= n_in, n_in = hi - 8 - lo (the trailer is read
//    by trailer32 alone);
//  * output: put(p, .) with p < size; copy(dst, src, n) with src + n <= dst and dst + n <= size (a match of
//    distance d at position p is checked for d <= p first, so src >= 0); flush(p) with p + kFlush <= size written;
//    flush_tail(p, n) with p + n = size;
//  * a violation ends the member with a Status, and so does a stream that runs past its last bit: every round of
//    every loop below takes at least one bit of input or ends, and the input is finite.
//
// Tables: a first level of kLitBits / kDistBits bits with 16-bit entries (symbol << 4 | length); a code longer than
// that is walked bit by bit over the counts per length and the symbols in canonical order.  A set of lengths is
// refused or accepted as build_table of wk_inflate.cpp does it (which is zlib's rule): over-subscribed never,
// incomplete only as one single code of one bit, empty only for distances.
//
// CRC-32 (the gzip polynomial, reflected) with state 0 and no final xor is linear in the message, so a message may
// be cut any way: crc0 of a concatenation is crc0(A) * x^(8 |B|) + crc0(B) (crc_mul, crc_xpow8), and crc_finish
// adds what the initial value and the final xor contribute.  CrcLanes is the cut the kernel uses: the output leaves
// in runs of kFlush bytes, lane l of 64 folds bytes [32 l, 32 l + 32) of every run into a state of its own (one
// multiplication per run for the gap to its next piece), and the states are joined once at the member's end.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WK_DI_FN __host__ __device__ __forceinline__
#else
#define WK_DI_FN inline
#endif

namespace wk {
namespace dinf {

enum Status : uint32_t {
    kOk = 0,
    kBadBlockType = 1,     // BTYPE 3
    kBadCodeLengths = 2,   // HLIT / HDIST out of range, a repeat with nothing before it or past the end, no end-of-block
                           // code, an over-subscribed or incomplete set
    kInvalidSymbol = 3,    // bits that are no code of the block's set, or a symbol the format does not define
    kDistanceTooFar = 4,   // a match that begins in front of the member's output
    kOutputOverrun = 5,    // the stream makes more bytes than the member states
    kInputOverrun = 6,     // the stream runs past the member's last bit
    kStoredLen = 7,        // LEN and NLEN of a stored block disagree
    kSizeMismatch = 8,     // the stream ends with fewer bytes than stated, or ISIZE is not what the spans say
    kCrcMismatch = 9,
    kBadSpans = 10,        // spans that are no member's (checked before anything is read)
};

constexpr uint32_t kLitBits = 10, kDistBits = 8, kClBits = 7;
constexpr uint32_t kFlush = 2048;            // bytes of output per run
constexpr uint32_t kLanes = 64, kPiece = kFlush / kLanes;
constexpr uint32_t kSymOver = 0xFFFEu, kSymNone = 0xFFFFu;

// the tables of the block being decoded (LDS on the device)
struct Tables {
    uint16_t lit[1u << kLitBits];
    uint16_t dst[1u << kDistBits];
    uint16_t cl[1u << kClBits];
    uint16_t lit_sym[288], dst_sym[32], cl_sym[20];
    uint16_t lit_cnt[16], dst_cnt[16], cl_cnt[16];
    uint16_t next_code[16], next_idx[16];
    uint8_t lens[320];
    uint8_t cl_lens[20];
};

// ---- CRC-32 in pieces -------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;

WK_DI_FN uint32_t crc_byte(uint32_t s, uint32_t b) {
    s ^= b;
    for (int k = 0; k < 8; ++k) s = (s >> 1) ^ (kCrcPoly & (0u - (s & 1u)));
    return s;
}
// four bytes at once, little-endian
WK_DI_FN uint32_t crc_word(uint32_t s, uint32_t w) {
    s ^= w;
    for (int k = 0; k < 32; ++k) s = (s >> 1) ^ (kCrcPoly & (0u - (s & 1u)));
    return s;
}
// a * b mod P (bit 31 is x^0)
WK_DI_FN uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) mod P
WK_DI_FN uint32_t crc_xpow8(uint64_t n) {
    uint32_t r = 0x80000000u, b = 0x00800000u;
    while (n) {
        if (n & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
        n >>= 1;
    }
    return r;
}
// crc0 of A followed by B, from crc0(A), crc0(B) and x^(8 |B|)
WK_DI_FN uint32_t crc_join(uint32_t a, uint32_t b, uint32_t xpow_b) { return crc_mul(a, xpow_b) ^ b; }
// gzip's CRC-32 of a message of n bytes from its crc0
WK_DI_FN uint32_t crc_finish(uint32_t s0, uint64_t n) { return s0 ^ crc_mul(0xFFFFFFFFu, crc_xpow8(n)) ^ 0xFFFFFFFFu; }

struct CrcLanes {
    // the gap between the end of a lane's piece and the start of its next one
    static WK_DI_FN uint32_t gap() { return crc_xpow8(kFlush - kPiece); }
    // from the end of lane l's piece to the end of its run
    static WK_DI_FN uint32_t rest(uint32_t lane) { return crc_xpow8(kFlush - (lane + 1u) * kPiece); }
    // lane's state over one more run: its kPiece bytes as kPiece / 4 little-endian words
    static WK_DI_FN uint32_t run(uint32_t s, uint32_t xgap, const uint32_t* w) {
        s = crc_mul(s, xgap);
        for (uint32_t j = 0; j < kPiece / 4; ++j) s = crc_word(s, w[j]);
        return s;
    }
    // how many bytes of a tail of n (< kFlush) bytes are lane l's
    static WK_DI_FN uint32_t tail_bytes(uint32_t lane, uint32_t n) {
        const uint32_t at = lane * kPiece;
        return n <= at ? 0u : (n - at < kPiece ? n - at : kPiece);
    }
    // what lane l adds to the member's crc0: its state over the full runs (s), the crc0 of its m bytes of the
    // tail (t); the xor over all lanes is the crc0 of the member
    static WK_DI_FN uint32_t last(uint32_t s, uint32_t lane, uint32_t xrest, uint32_t n_tail, uint32_t t, uint32_t m) {
        uint32_t r = crc_mul(s, crc_mul(xrest, crc_xpow8(n_tail)));
        if (m) r ^= crc_mul(t, crc_xpow8(n_tail - lane * kPiece - m));
        return r;
    }
};

// ---- the decoder ------------------------------------------------------------------------------
WK_DI_FN uint32_t len_base(uint32_t s) {   // s = symbol - 257 < 29
    return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1));
}
WK_DI_FN uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
WK_DI_FN uint32_t dist_base(uint32_t s) {  // s < 30
    return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1));
}
WK_DI_FN uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

WK_DI_FN uint32_t rev_bits(uint32_t c, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) {
        r = (r << 1) | (c & 1u);
        c >>= 1;
    }
    return r;
}

template <class Io>
struct Inflater {
    Io& io;
    Tables* t;
    uint64_t bb = 0;      // the next bc bits of the stream
    uint32_t bc = 0;
    uint32_t ip = 0;      // next compressed byte, from the stream's first
    uint32_t n_in;
    uint32_t pos = 0;     // bytes of output made
    uint32_t size;        // ... of the member, as stated
    uint32_t flushed = 0;

    WK_DI_FN Inflater(Io& io_, Tables* t_, uint32_t n_in_, uint32_t size_) : io(io_), t(t_), n_in(n_in_), size(size_) {}

    // more than 32 bits in the buffer wherever the input still has them
    WK_DI_FN void refill() {
        if (bc > 32) return;
        if (n_in - ip >= 4) {
            bb |= (uint64_t)io.in32(ip) << bc;
            ip += 4;
            bc += 32;
        } else {
            while (bc <= 56 && ip < n_in) {
                bb |= (uint64_t)io.in8(ip++) << bc;
                bc += 8;
            }
        }
    }
    WK_DI_FN bool take(uint32_t n, uint32_t& v) {   // n <= 16
        refill();
        if (bc < n) return false;
        v = (uint32_t)bb & ((1u << n) - 1u);
        bb >>= n;
        bc -= n;
        return true;
    }

    // The next symbol of a code: kSymOver where the input ends inside it, kSymNone for bits that are no code.
    // Takes at least one bit or returns kSymOver.
    WK_DI_FN uint32_t symbol(const uint16_t* tab, uint32_t P, const uint16_t* cnt, const uint16_t* syms) {
        refill();
        const uint32_t e = io.ld16(&tab[(uint32_t)bb & ((1u << P) - 1u)]);
        const uint32_t l = e & 15u;
        if (l) {
            if (l > bc) return kSymOver;
            bb >>= l;
            bc -= l;
            return e >> 4;
        }
        uint32_t code = 0, first = 0, index = 0;
        for (uint32_t len = 1; len <= 15; ++len) {
            if (!bc) return kSymOver;
            code |= (uint32_t)bb & 1u;
            bb >>= 1;
            --bc;
            const uint32_t count = io.ld16(&cnt[len]);
            if (code < first + count) return io.ld16(&syms[index + (code - first)]);
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
        return kSymNone;
    }

    // canonical code of lens[0, n): first-level table, counts per length, symbols in order
    WK_DI_FN bool build(uint16_t* tab, uint32_t P, uint16_t* cnt, uint16_t* syms, const uint8_t* lens, uint32_t n, bool need_one) {
        for (uint32_t l = 0; l < 16; ++l) io.st16(&cnt[l], 0);
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t l = io.ld8(&lens[s]);
            io.st16(&cnt[l], io.ld16(&cnt[l]) + 1u);
        }
        io.st16(&cnt[0], 0);
        int32_t left = 1;
        uint32_t total = 0, maxlen = 0, code = 0, idx = 0;
        for (uint32_t l = 1; l <= 15; ++l) {
            const uint32_t c = io.ld16(&cnt[l]);
            left = (left << 1) - (int32_t)c;
            if (left < 0) return false;
            total += c;
            if (c) maxlen = l;
            code = (code + io.ld16(&cnt[l - 1])) << 1;
            io.st16(&t->next_code[l], code);
            io.st16(&t->next_idx[l], idx);
            idx += c;
        }
        io.fill16(tab, 1u << P);
        if (total == 0) return !need_one;
        if (left > 0 && !(total == 1 && maxlen == 1)) return false;
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t l = io.ld8(&lens[s]);
            if (!l) continue;
            const uint32_t c = io.ld16(&t->next_code[l]), k = io.ld16(&t->next_idx[l]);
            io.st16(&t->next_code[l], c + 1u);
            io.st16(&t->next_idx[l], k + 1u);
            io.st16(&syms[k], s);
            if (l <= P) io.spread16(tab, rev_bits(c, l), 1u << l, 1u << P, (s << 4) | l);
        }
        return true;
    }

    WK_DI_FN Status fixed_tables() {
        for (uint32_t i = 0; i < 288; ++i) io.st8(&t->lens[i], i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (uint32_t i = 0; i < 32; ++i) io.st8(&t->lens[288 + i], 5);
        if (!build(t->lit, kLitBits, t->lit_cnt, t->lit_sym, t->lens, 288, true)) return kBadCodeLengths;
        if (!build(t->dst, kDistBits, t->dst_cnt, t->dst_sym, t->lens + 288, 32, false)) return kBadCodeLengths;
        return kOk;
    }

    WK_DI_FN Status dynamic_tables() {
        uint32_t h;
        if (!take(14, h)) return kInputOverrun;
        const uint32_t hlit = (h & 31u) + 257u, hdist = ((h >> 5) & 31u) + 1u, hclen = ((h >> 10) & 15u) + 4u;
        if (hlit > 286 || hdist > 30) return kBadCodeLengths;
        for (uint32_t i = 0; i < 19; ++i) io.st8(&t->cl_lens[i], 0);
        for (uint32_t i = 0; i < hclen; ++i) {
            uint32_t v;
            if (!take(3, v)) return kInputOverrun;
            // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
            const uint32_t at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 7 + ((i - 2) >> 1);
            io.st8(&t->cl_lens[at], v);
        }
        if (!build(t->cl, kClBits, t->cl_cnt, t->cl_sym, t->cl_lens, 19, true)) return kBadCodeLengths;
        const uint32_t n = hlit + hdist;
        uint32_t i = 0;
        while (i < n) {
            const uint32_t s = symbol(t->cl, kClBits, t->cl_cnt, t->cl_sym);
            if (s == kSymOver) return kInputOverrun;
            if (s == kSymNone) return kBadCodeLengths;
            if (s < 16) {
                io.st8(&t->lens[i++], s);
                continue;
            }
            uint32_t rep, val = 0, x;
            if (s == 16) {
                if (i == 0) return kBadCodeLengths;
                val = io.ld8(&t->lens[i - 1]);
                if (!take(2, x)) return kInputOverrun;
                rep = 3 + x;
            } else if (s == 17) {
                if (!take(3, x)) return kInputOverrun;
                rep = 3 + x;
            } else {
                if (!take(7, x)) return kInputOverrun;
                rep = 11 + x;
            }
            if (i + rep > n) return kBadCodeLengths;
            while (rep--) io.st8(&t->lens[i++], val);
        }
        if (io.ld8(&t->lens[256]) == 0) return kBadCodeLengths;
        if (!build(t->lit, kLitBits, t->lit_cnt, t->lit_sym, t->lens, hlit, true)) return kBadCodeLengths;
        if (!build(t->dst, kDistBits, t->dst_cnt, t->dst_sym, t->lens + hlit, hdist, false)) return kBadCodeLengths;
        return kOk;
    }

    WK_DI_FN void flush_full() {
        while (pos - flushed >= kFlush) {
            io.flush(flushed);
            flushed += kFlush;
        }
    }

    WK_DI_FN Status stored_block() {
        // the buffer holds the next bc bits of the stream: drop those of the current byte, hand the whole bytes back
        const uint32_t drop = bc & 7u;
        bb >>= drop;
        bc -= drop;
        ip -= bc >> 3;
        bb = 0;
        bc = 0;
        uint32_t v, w;
        if (!take(16, v) || !take(16, w)) return kInputOverrun;
        if ((v ^ 0xFFFFu) != w) return kStoredLen;
        ip -= bc >> 3;
        bb = 0;
        bc = 0;
        if (v > n_in - ip) return kInputOverrun;
        if (v > size - pos) return kOutputOverrun;
        while (v) {
            const uint32_t k = v < 256u ? v : 256u;
            io.copy_in(pos, ip, k);
            pos += k;
            ip += k;
            v -= k;
            flush_full();
        }
        return kOk;
    }

    WK_DI_FN Status coded_block() {
        for (;;) {
            const uint32_t s = symbol(t->lit, kLitBits, t->lit_cnt, t->lit_sym);
            if (s < 256) {
                if (pos >= size) return kOutputOverrun;
                io.put(pos++, s);
            } else if (s == 256) {
                return kOk;
            } else if (s < 286) {
                uint32_t x = 0;
                const uint32_t le = len_extra(s - 257);
                if (le && !take(le, x)) return kInputOverrun;
                const uint32_t len = len_base(s - 257) + x;
                const uint32_t d = symbol(t->dst, kDistBits, t->dst_cnt, t->dst_sym);
                if (d == kSymOver) return kInputOverrun;
                if (d >= 30) return kInvalidSymbol;
                const uint32_t de = dist_extra(d);
                x = 0;
                if (de && !take(de, x)) return kInputOverrun;
                const uint32_t dist = dist_base(d) + x;
                if (dist > pos) return kDistanceTooFar;
                if (len > size - pos) return kOutputOverrun;
                // a match that overlaps its own output repeats the dist bytes before it: what has been written
                // is a source for what follows, so every round may copy as much as lies behind it
                uint32_t done = 0;
                while (done < len) {
                    const uint32_t room = done + dist, n = len - done < room ? len - done : room;
                    io.copy(pos + done, pos - dist, n);
                    done += n;
                }
                pos += len;
            } else {
                return s == kSymOver ? kInputOverrun : kInvalidSymbol;
            }
            flush_full();
        }
    }

    // The whole member.  crc0 of the output is the Io's to give (it saw every byte leave).
    WK_DI_FN Status run() {
        for (;;) {
            uint32_t h;
            if (!take(3, h)) return kInputOverrun;
            const uint32_t btype = h >> 1;
            Status st;
            if (btype == 0) {
                st = stored_block();
            } else if (btype == 3) {
                return kBadBlockType;
            } else {
                st = btype == 1 ? fixed_tables() : dynamic_tables();
                if (st == kOk) st = coded_block();
            }
            if (st != kOk) return st;
            if (h & 1u) break;
        }
        if (pos != size) return kSizeMismatch;
        io.flush_tail(flushed, pos - flushed);
        if (io.trailer32(1) != size) return kSizeMismatch;
        if (crc_finish(io.crc0(pos - flushed), size) != io.trailer32(0)) return kCrcMismatch;
        return kOk;
    }
};

}  // namespace dinf
}  // namespace wk
