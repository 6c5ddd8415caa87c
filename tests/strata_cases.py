"""Inputs of the strata-join cases of tests/golden/vectors/strata_device.json:
hand-written read -> stratum maps (`map_cases`), the reads that probe them
(`probes`) and `--coords --stratify` commands on them (`cli_cases`), rebuilt
from seeds both by tests/golden/make_strata_reference.py (which runs the
reference on them) and by tests/test_strata_host.py / tests/test_gpu_strata.py.
Only what the reference makes of them is committed: per map the dict of
`workflow.read_strata` and the labels in order of first appearance, per command
its tables or its error.

Maps are bytes: \\r, \\v, \\f and a missing last newline are what the cases
are about.  A probe is (QNAME, mate), mate 0 | 1 | 2; the reference looks
QNAME, QNAME/1 or QNAME/2 up (`probe_key`)."""
import hashlib
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
LABEL_CAP = 1 << 16         # labels the device's table accepts (half of kStrataLabelSlots)
LABELS5 = ('soil', 'gut', 'reef', 'skin', 'air')

# the reasons for which the device leaves a map to the host's join
CAP, CR_KEY, CR_LABEL, TAIL = 'labels', 'cr-key', 'cr-label', 'tail'


def _lines(rows):
    return b''.join(r + b'\n' for r in rows)


def _clean(seed, n=300, name='c'):
    rng = random.Random(seed)
    return _lines(f'{name}{i:04d}\t{rng.choice(LABELS5)}'.encode()
                  for i in range(n))


def _near():
    """Every key on three consecutive lines.  Of every four keys one ends on
    the label of its first line, one starts on GONE -- which no key keeps."""
    rows = []
    for i in range(80):
        k = f'n{i:03d}'
        labs = (('A', 'B', 'C'), ('A', 'B', 'A'), ('GONE', 'B', 'C'),
                ('C', 'GONE', 'B'))[i % 4]
        rows += [f'{k}\t{x}'.encode() for x in labs]
    return _lines(rows)


def _far():
    """The same keys again more than 256 lines and more than 4096 bytes later
    (another workgroup, another tile of the line scan), with duplicates next
    to each other in front of and behind those distances."""
    keys = [f'f{i:02d}' for i in range(12)]

    def filler(tag):
        return [f'{tag}{i:04d}\tfilling-label-{i % 3}'.encode()
                for i in range(300)]
    rows = [f'{k}\tfirst'.encode() for k in keys]
    rows += [f'{k}\tsecond'.encode() for k in keys[:4]]         # near, in front
    rows += filler('x')
    rows += [f'{k}\tthird{i % 2}'.encode() for i, k in enumerate(keys[2:10])]
    rows += filler('y')
    rows += [f'{k}\tfourth'.encode() for k in keys[6:]]
    rows += [f'{k}\tfirst'.encode() for k in keys[8:10]]        # near, behind
    rows += [f'{keys[11]}\tlast'.encode()]
    return _lines(rows)


def _hot():
    rng = random.Random(31)
    return _lines(f'hot{rng.randrange(3)}\tH{rng.randrange(4)}'.encode()
                  for _ in range(20000))


def _columns():
    """Lines that are no pair between good ones; each carries a label (BAD*)
    or a key (bad*) that no good line has."""
    rng = random.Random(41)
    bad = [b'bad0 BAD0', b'bad1\tBAD1\tBAD1b', b'bad2\tBAD2\t\tBAD2c',
           b'bad3\tBAD3\t', b'', b'    ', b'bad4\t\tBAD4', b'\t\tBAD5',
           b'bad6\tBAD6\tx\ty', b'notab']
    rows = []
    for i in range(60):
        rows.append(f'g{i:03d}\t{rng.choice(LABELS5[:3])}'.encode())
        if i % 6 == 2:
            rows.append(bad[(i // 6) % len(bad)])
    return _lines(rows)


def _strip():
    rows = [b's00\tA ', b's01\tA \v\f', b's02\tA\f ', b's03\tA B', b's04\t A',
            b's05\t', b's06\t   ', b's07\tA', b's08\tA  B  ', b's09\t \vA',
            b's10\tB\v', b's11\t\f', b's12\tA\vB', b's13\tB \f \v ']
    return _lines(rows)


def _keys():
    rows = [b'\tE', b' k1\tLEAD', b'k1 \tTRAIL', b'k1\tBARE']
    abc = 'qwertyuiopasdfghjklzxcvbnm'
    for n in list(range(1, 18)) + [23, 24, 25]:
        rows.append(f'{abc[:n]}\tlen{n:02d}'.encode())
    base = 'ABCDEFGHIJKL'
    rows.append(f'{base}\tbase'.encode())
    for at in (0, 7, 8, len(base) - 1):
        rows.append(f'{base[:at]}#{base[at + 1:]}\tat{at:02d}'.encode())
    for k in ('r7', 'r7/', 'r7/1', 'r7/1x', 'r7/2'):
        rows.append(f'{k}\tchain[{k}]'.encode())
    rows.append(b'solo/1\tSOLO')
    # mates whose id ends around the 8 bytes of a hash round
    for n in range(4, 10):
        for m in (1, 2):
            rows.append(f'{"mnopqrstu"[:n]}/{m}\tmate{n}{m}'.encode())
    return _lines(rows)


def _few(n):
    return _lines(f'w{i:03d}\tL{i % 7}'.encode() for i in range(n))


def _cap(n):
    return _lines(b'read%06d\tL%05d' % (i, i) for i in range(n))


def cap_dict(n):
    """What the map `_cap(n)` says (its sha256 is what the fixture holds)."""
    return {f'read{i:06d}': f'L{i:05d}' for i in range(n)}


def dict_digest(d):
    return hashlib.sha256(''.join(
        f'{k}\t{v}\n' for k, v in sorted(d.items())).encode()).hexdigest()


def gold_map(gold, name):
    """(dict, labels in order) the fixture ``gold`` holds for the map case;
    the two maps around the label cap are rebuilt and checked against their
    digest, a map without pairs gives ({}, [])."""
    g = gold['maps'][name]
    if isinstance(g['strata'], list):           # ['ValueError', message]
        return {}, []
    if name.startswith('labels-'):
        want = cap_dict(g['labels']['count'])
        assert dict_digest(want) == g['strata']['sha256'] and \
            len(want) == g['strata']['pairs']
        return want, list(want.values())
    return g['strata'], g['labels']


def _odd(line):
    """A small clean map with one odd line in the middle."""
    body = _clean(51, 60, 'o')
    rows = body.split(b'\n')[:-1]
    rows.insert(30, line)
    return _lines(rows)


def kept_maps():
    """{name: bytes} of the maps the device keeps."""
    with_cr = _columns() + _strip()
    out = {
        'clean': _clean(21),
        'last-wins-near': _near(),
        'last-wins-far': _far(),
        'hot-keys': _hot(),
        'columns': _columns(),
        'strip': _strip(),
        'keys': _keys(),
        'crlf': with_cr.replace(b'\n', b'\r\n'),
        'crlf-as-lf': with_cr,          # (the same map with \n: same labels)
        'open-end-pair': _clean(61, 40, 'e') + b'last\tEND \v',
        'open-end-nonpair': _clean(62, 40, 'e') + b'last\tEND\tmore',
        'labels-65536': _cap(LABEL_CAP),
        'no-pairs': b'no tab here\nbad1\tBAD1\tBAD1b\n\n   \nbad3\tBAD3\t\n',
        'empty': b'',
        'one-newline': b'\n',
    }
    for n in (1, 255, 256, 257):
        out[f'few-lines-{n}'] = _few(n)
    return out


NO_LABELS = ('no-pairs', 'empty', 'one-newline')


def handoff_maps():
    """{name: (bytes, the reason)} of the maps the device leaves to the host."""
    return {
        'labels-65537': (_cap(LABEL_CAP + 1), CAP),
        'cr-in-key': (_odd(b'ab\rcd\tX'), CR_KEY),
        'cr-in-label': (_odd(b'ocr\tX\rY'), CR_LABEL),
        'tail-1c': (_odd(b'otail\tX\x1c'), TAIL),
        'tail-1f': (_odd(b'otail\tX \x1f'), TAIL),
        'tail-nbsp': (_odd('otail\tX\u00a0'.encode()), TAIL),
        'tail-eacute': (_odd('otail\tX\u00e9'.encode()), TAIL),
    }


_MAPS = {}


def map_cases():
    """{name: bytes} of all of them (built once)."""
    if not _MAPS:
        _MAPS.update(kept_maps())
        _MAPS.update({k: v[0] for k, v in handoff_maps().items()})
    return dict(_MAPS)


def handoff_reasons(text):
    """The reasons the device has to leave the map to the host's join, by the
    rules csrc/wk_strata.hpp states: a \\r that is not the last byte of its
    line in a key or inside a label, a stripped label that ends in a byte
    str.rstrip() may have an opinion on (\\x1c-\\x1f, anything beyond ASCII),
    more than LABEL_CAP distinct labels."""
    why, labels = set(), set()
    rows = text.split(b'\n')
    if rows and rows[-1] == b'':
        rows.pop()
    for row in rows:
        key, tab, val = row.partition(b'\t')
        if b'\r' in (key if tab else key[:-1]):
            why.add(CR_KEY)
        if not tab or b'\t' in val:
            continue
        val = val.rstrip(b'\r \v\f\n')
        if val and (val[-1] >= 0x80 or 0x1c <= val[-1] <= 0x1f):
            why.add(TAIL)
        if b'\r' in val:
            why.add(CR_LABEL)
        labels.add(val)
    if len(labels) > LABEL_CAP:
        why.add(CAP)
    return why


# ---- probes -------------------------------------------------------------------
def _is_qname(key):
    return bool(key) and key[:1] != b'@' and b'\r' not in key and \
        b'\t' not in key and b'\n' not in key


def _variants(key):
    """Ids next to ``key``: without its last byte, with one more, with one
    byte changed -- the first, the last, those at 7 and 8 (the end of the
    hash's first round)."""
    def changed(at):
        return key[:at] + (b'~' if key[at:at + 1] != b'~' else b'^') + \
            key[at + 1:]
    out = [key[:-1], key + b'~', changed(0), changed(len(key) - 1)]
    out += [changed(at) for at in (7, 8) if at < len(key)]
    return out


def probes(text, seed, most=None):
    """[(QNAME, mate)] for the map ``text``: every key that can be a QNAME (at
    most ``most`` of them, drawn by ``seed``) -- a key `x/1` or `x/2` also as
    the mates of `x`, and `x` by itself -- and their `_variants` in turn, one
    or two per key.  Consecutive probes have different QNAMEs but for the two
    mates of a pair."""
    rng = random.Random(seed)
    keys, pairs = [], []
    for row in text.splitlines():
        key, tab, val = row.partition(b'\t')
        if tab and _is_qname(key) and key not in keys[-3:]:
            keys.append(key)
            if b'\t' not in val:
                pairs.append(key)
    keys = list(dict.fromkeys(keys))
    pairs = list(dict.fromkeys(pairs))
    if most is not None and len(keys) > most:
        keys = rng.sample(keys, most)
        chosen = set(keys)
        pairs = [k for k in pairs if k in chosen]
    single, mated = list(keys), []
    for i, key in enumerate(pairs):
        alt = _variants(key)
        single.append(alt[i % len(alt)])
        if i % 3 == 2:
            single.append(alt[(i + 3) % len(alt)])
        if key[-2:] in (b'/1', b'/2') and _is_qname(key[:-2]):
            mated.append(key[:-2])
            single.append(key[:-2])
    single = [k for k in dict.fromkeys(single) if _is_qname(k)]
    units = [[(k.decode(), 0)] for k in single]
    units += [[(k.decode(), 1), (k.decode(), 2)]
              for k in dict.fromkeys(mated)]
    rng.shuffle(units)
    # no two neighbours with one QNAME
    for i in range(1, len(units)):
        if units[i][0][0] == units[i - 1][0][0]:
            for j in list(range(i + 1, len(units))) + list(range(i - 1)):
                a, b = units[j][0][0], units[i][0][0]
                around = {units[x][0][0] for x in (j - 1, j + 1)
                          if 0 <= x < len(units)}
                if a != units[i - 1][0][0] and b not in around and (
                        i + 1 >= len(units) or a != units[i + 1][0][0]):
                    units[i], units[j] = units[j], units[i]
                    break
    return [p for u in units for p in u]


def probe_key(probe):
    q, mate = probe
    return q if mate == 0 else f'{q}/{mate}'


def case_probes(name, text=None):
    """The probes of the map case ``name``."""
    if text is None:
        text = map_cases()[name]
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    got = probes(text, seed, 2000 if name.startswith('labels-') else None)
    if not got:     # (a map without keys: ids it cannot hold)
        got = [('nokey', 0), ('r7', 1), ('r7', 2), ('bad1', 0)]
    return got


FLAG = {0: 0, 1: 99, 2: 147}


def probe_sam(plist):
    """One SAM line per probe, on a genome of its own (P00000, P00001, ...):
    100 bases from position 1."""
    return ''.join(f'{q}\t{FLAG[m]}\tP{i:05d}\t1\t42\t100M\t=\t1\t0\t*\t*\n'
                   for i, (q, m) in enumerate(plist)).encode()


# ---- commands ------------------------------------------------------------------
GENOMES = 4


def coords_text():
    return ''.join(f'>G{g}\n' + ''.join(
        f'G{g}_{k}\t{1 + 150 * k}\t{200 + 150 * k}\n' for k in range(10))
        for g in range(GENOMES))


def _reads(plist, seed, mates, most=190):
    """(QNAME, mate, genome, position) of at most ``most`` of the probes (the
    two mates of a pair stay together).  No two reads of a file have one id
    (the reference makes one query of them, wherever they are in the file):
    where a probe (`x/1`, 0) stands next to a probe (`x`, 1), ``mates`` says
    which of the two the file keeps."""
    mated = {probe_key(p) for p in plist if p[1]}
    alone = {q for q, m in plist if not m}
    if mates:
        plist = [p for p in plist if p[1] or p[0] not in mated]
    else:
        plist = [p for p in plist if not p[1] or probe_key(p) not in alone]
    rng = random.Random(seed)
    units, i = [], 0
    while i < len(plist):
        n = 2 if plist[i][1] == 1 and i + 1 < len(plist) and \
            plist[i + 1] == (plist[i][0], 2) else 1
        units.append(plist[i:i + n])
        i += n
    order = list(range(len(units)))
    rng.shuffle(order)
    keep, n = [], 0
    for k in order:
        if n + len(units[k]) <= most:
            keep.append(k)
            n += len(units[k])
    keep.sort()
    return [(q, m, f'G{rng.randrange(GENOMES)}', rng.randrange(1, 1450))
            for k in keep for q, m in units[k]]


def reads_sam(reads, pad=False, star_at=None):
    """``pad``: SEQ and QUAL of 100 bytes; ``star_at``: behind that read's line
    one more of the same read with the CIGAR '*' (no length: no hit for the
    reference, and a line the device leaves to the host tokenizer)."""
    seq = ('ACGT' * 25, 'I' * 100) if pad else ('*', '*')
    rows = ['@HD\tVN:1.0\tSO:unsorted']
    for i, (q, m, g, pos) in enumerate(reads):
        rows.append(f'{q}\t{FLAG[m]}\t{g}\t{pos}\t42\t100M\t=\t1\t0'
                    f'\t{seq[0]}\t{seq[1]}')
        if i == star_at:
            rows.append(f'{q}\t{FLAG[m]}\t{g}\t{pos}\t42\t*\t=\t1\t0'
                        f'\t{seq[0]}\t{seq[1]}')
    return ('\n'.join(rows) + '\n').encode()


def reads_b6o(reads):
    return ''.join(f'{q}\t{g}\t98.5\t100\t0\t0\t1\t100\t{pos}\t{pos + 99}'
                   '\t1e-9\t200\n' for q, m, g, pos in reads if m == 0).encode()


def cli_cases():
    """[{'name', 'maps': the map cases of samples S1 and S2, 'fmt', 'pad',
    'star', 'route': 'device' | 'host' | 'error' | 'mixed'}]: `--coords
    --stratify` on two samples of at most 190 reads each.

    'mixed': padded lines, several blocks of 8 KB per sample, and one line
    with the CIGAR '*' in the middle of S1, whose block the device leaves to
    the host tokenizer while the others stay.  (A mapped line with both mate
    bits, FLAG 0xC0, sends its block to the host too -- but the reference
    raises IndexError on it, align.py:398, so no table could be compared.)"""
    def case(name, s1, s2=None, fmt='sam', route='device', **kw):
        return dict(dict(name=name, maps=(s1, s2 or s1), fmt=fmt, route=route,
                         pad=False, star=False), **kw)
    out = [
        case('clean', 'clean'),
        case('clean-b6o', 'clean', fmt='b6o'),
        case('last-wins', 'last-wins-near', 'last-wins-far'),
        case('hot-keys', 'hot-keys'),
        case('columns', 'columns'),
        case('strip', 'strip'),
        case('keys', 'keys'),
        case('crlf', 'crlf'),
        case('open-end', 'open-end-pair', 'open-end-nonpair'),
        case('few-lines', 'few-lines-1', 'few-lines-257'),
        case('labels-65536', 'labels-65536'),
    ]
    out += [case(name, name, route='host') for name in handoff_maps()]
    out += [case('no-pairs', 'clean', 'no-pairs', route='error'),
            case('empty', 'empty', 'clean', route='error'),
            case('mixed-routes', 'last-wins-near', pad=True, star=True,
                 route='mixed')]
    return out


def cli_files(case):
    """{relative path: bytes} of the case's files."""
    maps = map_cases()
    files = {'coords.txt': coords_text().encode()}
    for k, name in enumerate(case['maps']):
        s = f'S{k + 1}'
        reads = _reads(case_probes(name, maps[name]), 7 * k + len(name),
                       k == 0)
        if case['fmt'] == 'b6o':
            files[f'aln/{s}.b6o'] = reads_b6o(reads)
        else:
            files[f'aln/{s}.sam'] = reads_sam(
                reads, case['pad'],
                len(reads) // 2 if case['star'] and k == 0 else None)
        files[f'strata/{s}.txt'] = maps[name]
    return files


def write_cli(case, root):
    """The case's files under ``root``; returns workflow's keyword arguments
    (all but ``output_fp``)."""
    for rel, data in cli_files(case).items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(data)
    return dict(input_fp=os.path.join(root, 'aln'), input_fmt=case['fmt'],
                output_fmt=False, coords_fp=os.path.join(root, 'coords.txt'),
                strata_dir=os.path.join(root, 'strata'))


def run_cli(workflow, case, root):
    """Run ``workflow`` on the case: {'tables': {file name: text}} or
    {'error': [type name, message]} (the shape of `logred_cases.run_case`)."""
    import contextlib
    import io
    args = write_cli(case, root)
    out = os.path.join(root, 'out')
    args['output_fp'] = out
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            workflow(**args)
    except Exception as e:                  # noqa: BLE001 (the reference's own)
        return {'error': [type(e).__name__, str(e)]}
    if os.path.isdir(out):
        return {'tables': {fn: open(os.path.join(out, fn), newline='').read()
                           for fn in sorted(os.listdir(out))}}
    with open(out, newline='') as f:
        return {'tables': {'out': f.read()}}


# ---- what the cases promise ------------------------------------------------------
def map_dict(text):
    """The map as the package's own Python reader sees it (the reference's
    reading is the fixture's)."""
    import io
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from woltka_amd.file import read_map_uniq
    return dict(read_map_uniq(io.TextIOWrapper(io.BytesIO(text),
                                               encoding='utf-8')))


def check_inputs():
    kept, odd = kept_maps(), handoff_maps()
    for name, text in map_cases().items():
        rows = text.count(b'\n')
        if name.startswith('labels-'):
            # (18 bytes a line: about 1.2 MB, the largest input there is)
            assert rows in (LABEL_CAP, LABEL_CAP + 1) and \
                len(text) == 18 * rows, name
        elif name == 'hot-keys':
            assert rows == 20000 and len(text) < 1 << 20, name
        else:
            assert rows <= 700, (name, rows)
    for n in (1, 255, 256, 257):
        assert kept[f'few-lines-{n}'].count(b'\n') == n
    assert kept['crlf'].count(b'\r\n') == kept['crlf'].count(b'\n') == \
        kept['crlf'].count(b'\r') == kept['crlf-as-lf'].count(b'\n')
    assert not kept['open-end-pair'].endswith(b'\n')
    assert not kept['open-end-nonpair'].endswith(b'\n')
    # far: the keys come back in another workgroup and another tile
    far = kept['last-wins-far']
    at = [i for i, r in enumerate(far.split(b'\n')) if r.startswith(b'f02\t')]
    off = [far.index(b'f02\t'), far.rindex(b'f02\t')]
    assert len(at) >= 3 and at[1] - at[0] < 256 < at[2] - at[1] and \
        off[1] - off[0] > 4096
    for name, text in kept.items():
        assert handoff_reasons(text) == set(), name
    for name, (text, why) in odd.items():
        assert handoff_reasons(text) == {why}, (name, handoff_reasons(text))
    for name, text in map_cases().items():
        plist = case_probes(name, text)
        assert len(set(plist)) == len(plist), name
        for a, b in zip(plist, plist[1:]):
            assert a[0] != b[0] or (a[1], b[1]) == (1, 2), (name, a, b)
        for i, (q, m) in enumerate(plist):
            if m == 1:
                assert plist[i + 1] == (q, 2), (name, q)
        if name in NO_LABELS or name not in kept:
            continue
        have = map_dict(text)
        there = sum(probe_key(p) in have for p in plist)
        assert there >= 0.4 * len(plist) and \
            len(plist) - there >= 0.4 * len(plist), (name, there, len(plist))
    # a label only overridden lines name; the empty label; the chain of prefixes
    near = map_dict(kept['last-wins-near'])
    assert b'\tGONE\n' in kept['last-wins-near'] and \
        'GONE' not in near.values()
    assert '' in map_dict(kept['strip']).values()
    keys = map_dict(kept['keys'])
    assert {'', ' k1', 'k1 ', 'k1', 'r7', 'r7/', 'r7/1', 'r7/1x', 'r7/2',
            'solo/1'} <= set(keys) and 'solo' not in keys
    pk = case_probes('keys')
    for want in (('r7', 0), ('r7', 1), ('r7', 2), ('r7/1', 0), ('solo', 0),
                 ('solo', 1), ('solo', 2)):
        assert want in pk, want
    for case in cli_cases():
        files = cli_files(case)
        for k, v in files.items():
            if k.endswith('.sam'):
                ids = [probe_key((r.split(b'\t')[0].decode(),
                                  int(r.split(b'\t')[1]) >> 6 & 3))
                       for r in v.split(b'\n')[1:-1]
                       if r.split(b'\t')[5] != b'*']
                assert len(set(ids)) == len(ids), (case['name'], k)
        n = sum(v.count(b'\n') for k, v in files.items()
                if k.startswith('aln/'))
        assert 0 < n < 400, (case['name'], n)
        if case['route'] == 'mixed':
            assert all(len(v) > 3 << 13 for k, v in files.items()
                       if k.startswith('aln/'))
