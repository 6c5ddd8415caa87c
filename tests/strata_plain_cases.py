"""Inputs of the plain `--stratify` cases of
tests/golden/vectors/strata_plain_device.json: commands that classify subject
alignments (no `--coords`) stratified by a read -> stratum map per sample,
rebuilt from seeds both by tests/golden/make_strata_plain_reference.py (which
runs the reference on them) and by tests/test_strata_plain_host.py /
tests/test_gpu_strata_plain.py.  Only what the reference makes of a command is
committed: its tables or its error.

The maps and the reads that probe them are those of tests/strata_cases.py (the
join is blind to the format of the alignments: what a read's label is stands in
tests/golden/vectors/strata_device.json); the subjects are genomes of the
bundled taxonomy (tests/sizes_cases.py)."""
import gzip
import os
import random

import sizes_cases as SC
import strata_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
WIDE = 4096                 # WK_MAX_K + 1: subjects of a read the device leaves to the host
SMALL_BLOCK = 1 << 13       # DTOK_BLOCK of the cases cut into several blocks


def _only_mate1():
    """Only the first mates of the reads p00 .. p39."""
    return b''.join(f'p{i:02d}/1\tM{i % 3}\n'.encode() for i in range(40))


def own_maps():
    """{name: bytes} of the maps these cases add to `strata_cases.map_cases`."""
    return {'only-mate1': _only_mate1(),
            'clean-wide': T._clean(71, 300, 'c') + b'wide\tgut\n'}


_MAPS = {}


def maps():
    if not _MAPS:
        _MAPS.update(T.map_cases())
        _MAPS.update(own_maps())
    return _MAPS


# ---- reads -------------------------------------------------------------------
def _subjects(rng, pool):
    k = 1 if rng.random() < 0.55 else rng.randint(2, 5)
    return rng.sample(pool, k)


def probe_reads(name, seed, mates, pool, most=190):
    """[(QNAME, mate, subjects)] over the probes of the map ``name``: at most
    ``most`` reads, no two with one id (`strata_cases._reads`)."""
    rng = random.Random(seed + 1000)
    return [(q, m, _subjects(rng, pool)) for q, m, _, _ in T._reads(
        T.case_probes(name, maps()[name]), seed, mates, most) if q != 'wide']


def triple_reads(pool):
    """Every QNAME as one run of an unpaired read and both mates; a few of
    one mate alone."""
    rng = random.Random(77)
    out = []
    for i in range(44):
        for m in ((0, 1, 2) if i % 5 else (2,) if i % 2 else (1,)):
            out.append((f'p{i:02d}', m, _subjects(rng, pool)))
    return out


def stranger_reads(pool):
    """Reads none of which any map of the cases holds."""
    rng = random.Random(78)
    return [(f'z{i:04d}', 0, _subjects(rng, pool)) for i in range(150)]


def as_sam(recs, pad=False, wide_at=None, wide=None):
    """A line per (read, subject); of every seventh read the first subject
    twice.  ``pad``: SEQ and QUAL of 100 bytes.  ``wide``: subjects of one
    more read, `wide`, behind read ``wide_at`` (short lines)."""
    seq = ('ACGT' * 25, 'I' * 100) if pad else ('*', '*')
    rows = ['@HD\tVN:1.0\tSO:unsorted']
    for i, (q, m, subs) in enumerate(recs):
        for j, s in enumerate(subs + subs[:1] if i % 7 == 3 else subs):
            rows.append(f'{q}\t{T.FLAG[m]}\t{s}\t{1 + 7 * i + j}\t42\t50M\t*'
                        f'\t0\t0\t{seq[0]}\t{seq[1]}')
        if i == wide_at:
            rows += [f'wide\t0\t{s}\t{1 + j}\t42\t50M\t*\t0\t0\t*\t*'
                     for j, s in enumerate(wide)]
    return ('\n'.join(rows) + '\n').encode()


def _flat(recs):
    return [(q, subs) for q, m, subs in recs if m == 0]


RENDER = {'sam': lambda recs: as_sam(recs),
          'b6o': lambda recs: SC.as_b6o(_flat(recs)).encode(),
          'paf': lambda recs: SC.as_paf(_flat(recs)).encode(),
          'map': lambda recs: SC.as_map(_flat(recs)).encode()}


def wide_subjects():
    return [f'W{i:04d}' for i in range(WIDE)]


def wide_taxmap(pool):
    """The bundled genome -> taxon map with the subjects of the wide read on
    the taxa of ``pool``'s genomes in turn."""
    with open(os.path.join(SC.TAX, 'taxid.map')) as f:
        text = f.read()
    tax = dict(line.split() for line in text.splitlines() if line.strip())
    return (text + ''.join(f'{w}\t{tax[pool[i % len(pool)]]}\n'
                           for i, w in enumerate(wide_subjects()))).encode()


# ---- commands ------------------------------------------------------------------
def cases():
    """[{'name', 'files': {relative path: bytes}, 'kwargs': of
    workflow.workflow ('$TAX/...': a bundled file, other values that name a
    file of the case or the directories 'aln' / 'strata': under the case's
    root), 'route': 'device' | 'host' | 'error' | 'mixed', 'block': DTOK_BLOCK
    or None}] -- two samples S1 and S2 of at most 190 reads each but for the
    read of `WIDE` subjects of 'mixed-routes'; a file whose name ends in .gz
    is written through gzip."""
    G = SC.ranked_genomes()
    out = []

    def case(name, s1, s2=None, fmt='sam', route='device', block=None,
             reads=None, ext=None, pad=False, pool=None, files=None, **kw):
        names = (s1, s2 or s1)
        pool = pool or G
        ff = dict(files or {})
        for k, mp in enumerate(names):
            s = f'S{k + 1}'
            recs = (reads or {}).get(s) or probe_reads(
                mp, 7 * k + len(mp),
                fmt == 'sam' and (k == 0 or mp == 'keys'), pool)
            text = as_sam(recs, pad) if fmt == 'sam' else RENDER[fmt](recs)
            ff.setdefault(f'aln/{s}.{ext or fmt}', text)
            ff[f'strata/{s}.txt'] = maps()[mp]
        kwargs = dict(input_fp='aln', input_fmt=fmt, output_fmt=False,
                      strata_dir='strata', ranks='none,genus')
        kwargs.update(SC.TREE)
        kwargs.update(kw)
        out.append(dict(name=name, files=ff, kwargs=kwargs, route=route,
                        block=block))

    # one command per format (S2's map holds mates: the SAM file has them)
    for fmt in ('sam', 'b6o', 'paf', 'map'):
        case(f'fmt-{fmt}', 'clean', 'keys', fmt=fmt)
    # the assigners
    case('sam-none', 'last-wins-near', 'columns', ranks='none')
    case('sam-genus', 'last-wins-near', 'columns', ranks='genus')
    case('sam-free', 'last-wins-near', 'columns', ranks='free')
    case('sam-mixed', 'last-wins-near', 'columns',
         ranks='none,free,phylum,genus')
    case('sam-uniq', 'last-wins-near', 'columns', ranks='genus', uniq=True)
    case('sam-major', 'last-wins-near', 'columns', ranks='genus', major=80)
    # `--trim-sub`: several names, one subject
    case('trimsub', 'strip', 'keys', ranks='genus,species', trimsub='_',
         pool=[f'{g}_{k}' for g in G[:40] for k in (1, 2, 3)])
    case('exclude', 'clean', 'columns', pool=G[:30],
         exclude=','.join(G[1:4]))
    # one QNAME as an unpaired read and both mates, the map holds the first
    case('mates', 'only-mate1', 'keys',
         reads={'S1': triple_reads(G)})
    # a sample none of whose reads is in its map
    case('strangers', 'clean', 'clean', reads={'S2': stranger_reads(G)})
    # two maps of different sizes, the second read while the first is joined
    case('two-maps', 'hot-keys', 'few-lines-257')
    case('gz', 'clean', 'strip', ext='sam.gz')
    case('blocks', 'clean', 'last-wins-far', pad=True, block=SMALL_BLOCK)
    # one read of more subjects than a count key can say in the middle of S1:
    # its block is the host's, the others stay on the device
    recs = probe_reads('clean-wide', 5, False, G)
    case('mixed-routes', 'clean-wide', 'clean', route='mixed',
         block=SMALL_BLOCK, pad=True, ranks='phylum,genus',
         map_fps=['tax.map'],
         files={'aln/S1.sam': as_sam(recs, True, len(recs) // 2,
                                     wide_subjects()),
                'tax.map': wide_taxmap(G)})
    # a map without pairs
    case('no-pairs', 'clean', 'no-pairs', route='error')
    # the maps the device leaves to the host's join
    for name in T.handoff_maps():
        case(f'handoff-{name}', name, route='host', ranks='genus')
    return out


def write_case(case, root):
    """The case's files under ``root``; returns the keyword arguments of
    `workflow` with the paths made real (all but ``output_fp``)."""
    for rel, data in case['files'].items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if rel.endswith('.gz'):
            with gzip.GzipFile(path, 'wb', mtime=0) as f:
                f.write(data)
        else:
            with open(path, 'wb') as f:
                f.write(data)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return os.path.join(SC.TAX, v[5:])
        if isinstance(v, str) and (v in ('aln', 'strata') or
                                   v in case['files']):
            return os.path.join(root, v)
        return v
    return {k: real(v) for k, v in case['kwargs'].items()}


def tables_of(out):
    """{file name: text} of what a command wrote to ``out``."""
    if os.path.isdir(out):
        return {fn: open(os.path.join(out, fn), newline='').read()
                for fn in sorted(os.listdir(out))}
    with open(out, newline='') as f:
        return {'out': f.read()}


def run_case(workflow, case, root, **more):
    """Run ``workflow`` on the case: {'tables': {file name: text}} or
    {'error': [type name, message]}."""
    import contextlib
    import io
    args = write_case(case, root)
    args.update(more)
    out = os.path.join(root, 'out')
    args['output_fp'] = out
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            workflow(**args)
    except Exception as e:                  # noqa: BLE001 (the reference's own)
        return {'error': [type(e).__name__, str(e)]}
    return {'tables': tables_of(out)}


# ---- what the cases promise ------------------------------------------------------
def sam_reads(text):
    """[(read id, subjects in order, each once)] of a SAM text of the cases."""
    mate = {v: k for k, v in T.FLAG.items()}
    out = {}
    for row in text.decode().splitlines():
        if row[0] == '@':
            continue
        q, flag, s = row.split('\t')[:3]
        out.setdefault(T.probe_key((q, mate[int(flag)])), {})[s] = True
    return [(q, list(subs)) for q, subs in out.items()]


def check_inputs():
    cs = {c['name']: c for c in cases()}
    assert len(cs) == len(cases())
    for name, c in cs.items():
        aln = {k: v for k, v in c['files'].items() if k.startswith('aln/')}
        assert len(aln) == 2, name
        for k, v in aln.items():
            rows = v.count(b'\n')
            if name == 'mixed-routes' and k == 'aln/S1.sam':
                assert WIDE < rows < WIDE + 900
            else:
                assert 0 < rows < 900, (name, k, rows)
            if k.endswith(('.sam', '.sam.gz')):
                # a read's lines are neighbours: no id in two runs
                ids = [tuple(r.split(b'\t')[:2]) for r in v.split(b'\n')[1:-1]]
                runs = [q for i, q in enumerate(ids)
                        if i == 0 or ids[i - 1] != q]
                assert len(set(runs)) == len(runs), (name, k)
        if c['block']:
            assert all(len(v) > 3 * c['block'] for v in aln.values()), name
    # the mates of the 'mates' case: runs of three reads, the map holds one
    reads = dict(sam_reads(cs['mates']['files']['aln/S1.sam']))
    held = T.map_dict(maps()['only-mate1'])
    assert {'p01', 'p01/1', 'p01/2'} <= set(reads) and 'p01/1' in held and \
        'p01' not in held and 'p01/2' not in held
    # nobody of S2 of 'strangers' is in its map
    held = T.map_dict(maps()['clean'])
    reads = sam_reads(cs['strangers']['files']['aln/S2.sam'])
    assert len(reads) == 150 and not any(q in held for q, _ in reads)
    # about half of the other samples' reads are
    reads = sam_reads(cs['sam-genus']['files']['aln/S1.sam'])
    held = T.map_dict(maps()['last-wins-near'])
    assert 0.3 * len(reads) < sum(q in held for q, _ in reads) < \
        0.7 * len(reads)
    # the wide read: in its map, `WIDE` subjects, all with a genus
    reads = dict(sam_reads(cs['mixed-routes']['files']['aln/S1.sam']))
    assert len(reads['wide']) == WIDE and \
        'wide' in T.map_dict(maps()['clean-wide'])
    assert cs['gz']['files'].keys() >= {'aln/S1.sam.gz', 'aln/S2.sam.gz'}
