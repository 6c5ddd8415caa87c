"""Member chains for the device inflater's tests (test_dinflate_core_host.py,
test_gpu_dinflate.py): what zlib writes at several levels and strategies, and
streams it never writes, assembled bit by bit.

A case is `(name, blob, lo, hi, off, want, status)`: the chain's bytes, per
member the start of its DEFLATE stream, its end, and the running sum of the
stated sizes; the bytes expected (from zlib, never from this package's own
decoders) and per member the status expected (0, a `wk::dinf::Status`, or
ANY for "not 0").  Every good member is first inflated with zlib and held
against the bytes it was made from, so a fixture that is itself invalid cannot
pass for a decoder bug."""
import random
import struct
import zlib

ANY = 0xFFFFFFFF
(OK, BAD_BLOCK_TYPE, BAD_CODE_LENGTHS, INVALID_SYMBOL, DISTANCE_TOO_FAR,
 OUTPUT_OVERRUN, INPUT_OVERRUN, STORED_LEN, SIZE_MISMATCH, CRC_MISMATCH,
 BAD_SPANS) = range(11)

BC_HEAD = 18
WK_HEAD = 20


def sam_text(n, seed=1):
    rnd = random.Random(seed)
    return b''.join(b'R%09d\t%d\tT%07d\t%d\t42\t%dM\t*\t0\t0\t*\t*\n' % (
        i // 3, rnd.choice((0, 16, 99, 147)), rnd.randrange(100000),
        rnd.randrange(1, 10 ** 6), rnd.randrange(30, 151)) for i in range(n))


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def bgzf(body, data, crc=None, isize=None, bsize=None):
    """A BGZF member around DEFLATE stream `body`."""
    size = BC_HEAD + len(body) + 8
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' +
            struct.pack('<H', (size if bsize is None else bsize) - 1) + body +
            struct.pack('<II', zlib.crc32(data) if crc is None else crc,
                        len(data) if isize is None else isize))


def wk_member(body, data):
    size = WK_HEAD + len(body) + 8
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x08\x00WK\x04\x00' +
            struct.pack('<I', size) + body +
            struct.pack('<II', zlib.crc32(data), len(data)))


# ---- streams written bit by bit ------------------------------------------
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43,
            51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257,
             385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0) + tuple(k for k in range(1, 14) for _ in (0, 1))
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code for the 19 code-length symbols: every length written plainly
CL_LENS = [4] * 13 + [5] * 6


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code of `lens`."""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):           # n bits, the lowest first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, cn):             # a Huffman code, its highest bit first
        c, n = cn
        for i in range(n - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def stored(self, data, final=False, nlen=None):
        self.bits(int(final), 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data

    def header(self, lit_lens, dist_lens, final=False, cl_lens=CL_LENS,
               plan=None):
        """BFINAL, BTYPE = 2 and the code lengths; `plan`: the code-length
        symbols to write, as (symbol, extra value) (default: one plain length
        per code)."""
        self.bits(int(final), 1)
        self.bits(2, 2)
        self.bits(len(lit_lens) - 257, 5)
        self.bits(len(dist_lens) - 1, 5)
        self.bits(19 - 4, 4)
        for s in CL_ORDER:
            self.bits(cl_lens[s], 3)
        cl = canonical(cl_lens)
        if plan is None:
            plan = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
        for s, x in plan:
            self.code(cl[s])
            if s >= 16:
                self.bits(x, (2, 3, 7)[s - 16])

    def tokens(self, toks, lit_lens, dist_lens):
        """Literals (ints), matches ((length, distance)) and the end of the
        block."""
        lit, dst = canonical(lit_lens), canonical(dist_lens)
        for t in toks:
            if isinstance(t, int):
                self.code(lit[t])
                continue
            ln, d = t
            s = max(i for i in range(29) if LEN_BASE[i] <= ln)
            if ln == 258:
                s = 28
            self.code(lit[257 + s])
            self.bits(ln - LEN_BASE[s], LEN_EXTRA[s])
            s = max(i for i in range(30) if DIST_BASE[i] <= d)
            self.code(dst[s])
            self.bits(d - DIST_BASE[s], DIST_EXTRA[s])
        self.code(lit[256])

    def fixed(self, toks, final=False):
        self.bits(int(final), 1)
        self.bits(1, 2)
        self.tokens(toks, FIXED_LIT, FIXED_DIST)

    def dynamic(self, toks, lit_lens, dist_lens, final=False):
        self.header(lit_lens, dist_lens, final)
        self.tokens(toks, lit_lens, dist_lens)

    def done(self):
        self.align()
        return bytes(self.out)


def lens_of(n, assigned):
    out = [0] * n
    for s, l in assigned.items():
        out[s] = l
    return out


def _pattern(n, seed):
    return bytes(random.Random(seed).randrange(256) for _ in range(n))


def hand_built():
    """{name: DEFLATE stream}."""
    out = {}
    # a match of 258 at distance 32 768 = all that has been written; later one at 32 768 from the window's edge
    b = Bits()
    b.stored(_pattern(32768, 1))
    b.fixed([(258, 32768), 65, 66])
    b.stored(_pattern(7000, 2))
    b.fixed([(258, 32768), (3, 32768), 67], final=True)
    out['edge of the window'] = b.done()
    # codes of 15 bits: literal 'z' and the end of the block; distance symbols 14 and 15
    chain = {97 + i: i + 1 for i in range(13)}
    chain.update({257: 14, ord('z'): 15, 256: 15})
    dchain = {i: i + 1 for i in range(14)}
    dchain.update({14: 15, 15: 15})
    b = Bits()
    b.dynamic([97] * 300 + [98, 99, 109, ord('z'), (3, 129 + 7), ord('z'), (3, 193 + 40), 97],
              lens_of(258, chain), lens_of(16, dchain), final=True)
    out['codes of 15 bits'] = b.done()
    # one distance code (one bit), used
    lit = lens_of(259, {120: 1, 121: 2, 256: 3, 257: 4, 258: 4})
    b = Bits()
    b.dynamic([120, 121, (3, 1), (4, 1), 120], lit, [1], final=True)
    out['a single distance code'] = b.done()
    # no distance code at all, literals only
    b = Bits()
    b.dynamic([120, 121, 121, 120] * 20, lens_of(257, {120: 1, 121: 2, 256: 2}), [0], final=True)
    out['no distance code'] = b.done()
    # a length with 5 extra bits, a distance with 13
    b = Bits()
    b.stored(_pattern(30000, 3))
    lit = lens_of(286, {65: 2, 256: 2, 284: 2, 281: 3, 285: 3})
    dst = lens_of(30, {28: 1, 29: 2, 0: 2})
    b.dynamic([65, (250, 20000), (131 + 17, 24577 + 5000), 65, (258, 1), (227, 16385)], lit, dst, final=True)
    out['long extra bits'] = b.done()
    return out


def damaged_streams():
    """{name: (DEFLATE stream, status)} of streams that are wrong in themselves."""
    out = {}
    b = Bits()
    b.fixed([(3, 1), 65], final=True)
    out['first symbol is a match'] = (b.done(), DISTANCE_TOO_FAR)
    b = Bits()
    b.bits(1, 1)
    b.bits(3, 2)
    b.bits(0, 29)
    out['block type 3'] = (b.done(), BAD_BLOCK_TYPE)
    b = Bits()
    b.dynamic([65], lens_of(257, {65: 1, 66: 1, 256: 1}), [1], final=True)
    out['over-subscribed lengths'] = (b.done(), BAD_CODE_LENGTHS)
    b = Bits()
    lit = lens_of(257, {65: 1, 256: 1})
    b.header(lit, [1], final=True, plan=[(16, 0)] + [(l, 0) for l in lit + [1]])
    b.tokens([65], lit, [1])
    out['repeat with nothing before it'] = (b.done(), BAD_CODE_LENGTHS)
    b = Bits()
    b.stored(b'hello', final=True, nlen=5)
    out['LEN and NLEN disagree'] = (b.done(), STORED_LEN)
    return out


def chain(members):
    """A case from [(member bytes, head length, stated size, expected bytes or
    None, status, hi or None)]."""
    blob, lo, hi, off, want, status = b'', [], [], [0], b'', []
    for m, head, size, data, st, end in members:
        lo.append(len(blob) + head)
        hi.append(len(blob) + (len(m) if end is None else end))
        blob += m
        off.append(off[-1] + size)
        want += data if data is not None else b'\0' * size
        status.append(st)
    return blob, lo, hi, off, want, status


def good(data, body=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wk=False):
    """A member tuple for `chain`; the stream is checked against zlib here."""
    if body is None:
        body = raw_deflate(data, level, strategy)
    assert zlib.decompress(body, -15) == data
    if wk:
        return wk_member(body, data), WK_HEAD, len(data), data, OK, None
    return bgzf(body, data), BC_HEAD, len(data), data, OK, None


def good_cases():
    sam = sam_text(4000)
    rnd = _pattern(5000, 7)
    cases = []

    def add(name, members):
        cases.append((name,) + chain(members))

    add('stored', [good(sam[:3000], level=0)])
    b = Bits()
    b.stored(sam[:700])
    b.stored(b'')
    b.stored(sam[700:900], final=True)
    add('empty stored block between two', [good(sam[:900], b.done())])
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(sam[:500]) + c.flush(zlib.Z_SYNC_FLUSH)
    add('sync flush', [good(sam[:800], body + c.compress(sam[500:800]) + c.flush())])
    add('fixed', [good(sam[:5000], strategy=zlib.Z_FIXED)])
    for level in (1, 6, 9):
        add('dynamic level %d' % level, [good(sam[:60000], level=level)])
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(sam[:20000]) + c.flush(zlib.Z_FULL_FLUSH)
    b = Bits()
    b.out += body                         # (a full flush ends on a byte boundary, in an empty stored block)
    b.stored(rnd[:1000])
    b.fixed(list(b'fixed block here'), final=True)
    add('three blocks of different types', [good(sam[:20000] + rnd[:1000] + b'fixed block here', b.done())])
    add('one byte', [good(b'x')])
    add('empty members', [good(b''), good(sam[:100]), good(b''), good(sam[100:300]), good(b'')])
    add('run of one byte', [good(b'A' * 65280)])
    for name, body in hand_built().items():
        add(name, [good(zlib.decompress(body, -15), body)])
    add('random bytes', [good(rnd)])
    full = sam_text(1600, 5)[:65280]
    assert len(full) == 65280
    add('full BGZF member', [good(full)])
    period = _pattern(32000, 11)
    big = period * 33
    body = raw_deflate(big, 9)
    add('WK member of 1 MB, matches 32 000 back', [good(big, body, wk=True)])
    text = sam_text(1500, 9)
    many = []
    for i in range(300):
        many.append(good(b'%c' % (65 + i % 26)) if i % 2 == 0 else good(text[i * 7:i * 7 + 60000]))
    add('300 members', many)
    return cases


def damage_cases():
    sam = sam_text(1500, 4)
    left, right, mid = sam[:2000], sam[2000:5000], sam[5000:30000]
    body = raw_deflate(mid)
    cases = []

    def add(name, bad):
        cases.append((name,) + chain([good(left), bad, good(right)]))

    flipped = bytearray(body)
    flipped[len(body) // 2] ^= 0x10
    add('a flipped bit', (bgzf(bytes(flipped), mid), BC_HEAD, len(mid), None, ANY, None))
    add('CRC off by one bit', (bgzf(body, mid, crc=zlib.crc32(mid) ^ 0x400), BC_HEAD, len(mid), None, CRC_MISMATCH, None))
    add('ISIZE too small', (bgzf(body, mid, isize=len(mid) - 5), BC_HEAD, len(mid) - 5, None, OUTPUT_OVERRUN, None))
    add('ISIZE too large', (bgzf(body, mid, isize=len(mid) + 5), BC_HEAD, len(mid) + 5, None, SIZE_MISMATCH, None))
    m = bgzf(body, mid)
    add('member ends inside the stream', (m, BC_HEAD, len(mid), None, INPUT_OVERRUN, len(m) - 20))
    for name, (stream, st) in damaged_streams().items():
        add(name, (bgzf(stream, b'\0' * 10), BC_HEAD, 10, None, st, None))
    return cases


def crc_cases():
    data = _pattern(65280 * 2 + 77, 13)
    return [(data[:n], piece, zlib.crc32(data[:n]))
            for n in (0, 1, 63, 64, 65, 65280, len(data))
            for piece in (0, 1, 63, 64, 65, 65280)]


def write_file(path, cases, crcs):
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for name, blob, lo, hi, off, want, status in cases:
            nm = name.encode()
            f.write(struct.pack('<I', len(nm)) + nm)
            f.write(struct.pack('<Q', len(blob)) + blob)
            f.write(struct.pack('<I', len(lo)))
            for a, b in zip(lo, hi):
                f.write(struct.pack('<qq', a, b))
            f.write(struct.pack('<%dq' % len(off), *off))
            assert len(want) == off[-1]
            f.write(want)
            f.write(struct.pack('<%dI' % len(status), *status))
        f.write(struct.pack('<I', len(crcs)))
        for data, piece, crc in crcs:
            f.write(struct.pack('<Q', len(data)) + data + struct.pack('<II', piece, crc))
