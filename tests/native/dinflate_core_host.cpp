// The device inflater's core (csrc/wk_dinflate_core.hpp) on the CPU, over a file of cases that
// tests/test_dinflate_core_host.py writes.  Every member is decoded from a heap copy of exactly its own compressed
// span into a heap buffer of exactly its stated size, so AddressSanitizer ends the program on any access outside
// either; the CRC is folded by 64 lane states over runs of 2 KB, as the kernel folds it.
//
// File (little-endian): u32 cases; per case u32 name length, name, u64 blob length, blob, u32 members, lo / hi
// (i64 each) per member, members + 1 i64 off, off[members] expected bytes, u32 expected status per member
// (0xFFFFFFFF: any but 0).  Then u32 CRC cases; per case u64 length, bytes, u32 piece length, u32 expected CRC-32.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wk_dinflate_core.hpp"

using namespace wk::dinf;

struct HostIo {
    const unsigned char* in;   // the stream: n_in bytes, then the trailer
    unsigned char* out;
    uint32_t n_in;
    uint32_t crc_s[kLanes], crc_t[kLanes], xgap;

    uint32_t ld16(const uint16_t* p) const { return *p; }
    uint32_t ld8(const uint8_t* p) const { return *p; }
    void st16(uint16_t* p, uint32_t v) const { *p = (uint16_t)v; }
    void st8(uint8_t* p, uint32_t v) const { *p = (uint8_t)v; }
    void fill16(uint16_t* p, uint32_t n) const { std::memset(p, 0, 2 * (size_t)n); }
    void spread16(uint16_t* p, uint32_t start, uint32_t step, uint32_t end, uint32_t v) const {
        for (uint32_t i = start; i < end; i += step) p[i] = (uint16_t)v;
    }
    uint32_t in32(uint32_t ip) const {
        uint32_t v;
        std::memcpy(&v, in + ip, 4);
        return v;
    }
    uint32_t in8(uint32_t ip) const { return in[ip]; }
    uint32_t trailer32(uint32_t k) const {
        uint32_t v;
        std::memcpy(&v, in + n_in + 4 * k, 4);
        return v;
    }
    void put(uint32_t p, uint32_t b) const { out[p] = (unsigned char)b; }
    void copy(uint32_t dst, uint32_t src, uint32_t n) const {
        if (src + n > dst) std::abort();
        std::memcpy(out + dst, out + src, n);
    }
    void copy_in(uint32_t dst, uint32_t ip, uint32_t n) const { std::memcpy(out + dst, in + ip, n); }
    void flush(uint32_t p) {
        for (uint32_t l = 0; l < kLanes; ++l) {
            uint32_t w[kPiece / 4];
            std::memcpy(w, out + p + l * kPiece, kPiece);
            crc_s[l] = CrcLanes::run(crc_s[l], xgap, w);
        }
    }
    void flush_tail(uint32_t p, uint32_t n) {
        for (uint32_t l = 0; l < kLanes; ++l) {
            const uint32_t m = CrcLanes::tail_bytes(l, n);
            uint32_t t = 0;
            for (uint32_t k = 0; k < m; ++k) t = crc_byte(t, out[p + l * kPiece + k]);
            crc_t[l] = t;
        }
    }
    uint32_t crc0(uint32_t n_tail) const {
        uint32_t r = 0;
        for (uint32_t l = 0; l < kLanes; ++l)
            r ^= CrcLanes::last(crc_s[l], l, CrcLanes::rest(l), n_tail, crc_t[l], CrcLanes::tail_bytes(l, n_tail));
        return r;
    }
};

struct Reader {
    std::vector<unsigned char> b;
    size_t at = 0;
    template <typename T>
    T get() {
        T v;
        if (at + sizeof v > b.size()) {
            std::fprintf(stderr, "case file too short\n");
            std::exit(2);
        }
        std::memcpy(&v, b.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    const unsigned char* bytes(size_t n) {
        if (at + n > b.size()) {
            std::fprintf(stderr, "case file too short\n");
            std::exit(2);
        }
        const unsigned char* p = b.data() + at;
        at += n;
        return p;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    Reader r;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        unsigned char buf[1 << 16];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) r.b.insert(r.b.end(), buf, buf + k);
        std::fclose(f);
    }
    int failures = 0, members = 0;
    const uint32_t n_cases = r.get<uint32_t>();
    for (uint32_t c = 0; c < n_cases; ++c) {
        const uint32_t nl = r.get<uint32_t>();
        const std::string name((const char*)r.bytes(nl), nl);
        const uint64_t blob_n = r.get<uint64_t>();
        const unsigned char* blob = r.bytes(blob_n);
        const uint32_t n = r.get<uint32_t>();
        std::vector<int64_t> lo(n), hi(n), off(n + 1);
        for (uint32_t i = 0; i < n; ++i) {
            lo[i] = r.get<int64_t>();
            hi[i] = r.get<int64_t>();
        }
        for (uint32_t i = 0; i <= n; ++i) off[i] = r.get<int64_t>();
        const unsigned char* want = r.bytes((size_t)off[n]);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t want_st = r.get<uint32_t>();
            ++members;
            if (lo[i] < 0 || hi[i] - lo[i] < 8 || (uint64_t)hi[i] > blob_n || off[i + 1] < off[i]) {
                std::printf("FAIL %s member %u: spans of the case itself\n", name.c_str(), i);
                ++failures;
                continue;
            }
            const size_t span = (size_t)(hi[i] - lo[i]), size = (size_t)(off[i + 1] - off[i]);
            unsigned char* in = (unsigned char*)std::malloc(span);
            unsigned char* out = (unsigned char*)std::malloc(size ? size : 1);
            std::memcpy(in, blob + lo[i], span);
            std::memset(out, 0xEE, size ? size : 1);
            Tables* t = (Tables*)std::malloc(sizeof(Tables));
            std::memset(t, 0xEE, sizeof(Tables));
            HostIo io{};
            io.in = in;
            io.out = out;
            io.n_in = (uint32_t)(span - 8);
            io.xgap = CrcLanes::gap();
            Inflater<HostIo> inf(io, t, io.n_in, (uint32_t)size);
            const uint32_t st = inf.run();
            const bool st_ok = want_st == 0xFFFFFFFFu ? st != 0 : st == want_st;
            if (!st_ok) {
                std::printf("FAIL %s member %u: status %u, expected %d\n", name.c_str(), i, st, (int)want_st);
                ++failures;
            } else if (st == 0 && std::memcmp(out, want + off[i], size) != 0) {
                std::printf("FAIL %s member %u: bytes differ\n", name.c_str(), i);
                ++failures;
            }
            std::free(t);
            std::free(out);
            std::free(in);
        }
    }
    const uint32_t n_crc = r.get<uint32_t>();
    for (uint32_t c = 0; c < n_crc; ++c) {
        const uint64_t n = r.get<uint64_t>();
        const unsigned char* data = r.bytes(n);
        const uint32_t piece = r.get<uint32_t>(), want = r.get<uint32_t>();
        // pieces of `piece` bytes (one of n bytes for 0), each folded from 0, joined left to right
        uint32_t acc = 0;
        uint64_t at = 0;
        const uint64_t step = piece ? piece : (n ? n : 1);
        while (at < n) {
            const uint64_t k = n - at < step ? n - at : step;
            uint32_t s = 0;
            for (uint64_t i = 0; i < k; ++i) s = crc_byte(s, data[at + i]);
            acc = crc_join(acc, s, crc_xpow8(k));
            at += k;
        }
        const uint32_t got = crc_finish(acc, n);
        if (got != want) {
            std::printf("FAIL crc of %llu bytes in pieces of %u: %08x, expected %08x\n", (unsigned long long)n, piece, got, want);
            ++failures;
        }
    }
    std::printf("%u cases, %d members, %u crc cases, %d failures\n", n_cases, members, n_crc, failures);
    return failures ? 1 : 0;
}
