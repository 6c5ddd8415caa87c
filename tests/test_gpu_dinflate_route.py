"""Alignment files that are chains of gzip members stating their size (BGZF,
'WK') through the device text route with their text inflated on the device
(`blocks_members` in routes/device_text.py, `wk_dtok_inflate_ahead`).

The bundled goldens are rewritten as BGZF with members of 4 000 bytes of text,
so members end inside lines and inside runs of one query; blocks of 64 KB and
of 64 MB.  The tables must be the bundled ones byte for byte, with blocks
counted under ROUTES['dinflate'] and none handed to the host tokenizer;
WOLTKA_NO_DINFLATE=1 gives the same bytes the old way.  Further: a 'WK'
chain, a header that outlasts the first block, a run of one query longer than
a block, a chain with an ordinary gzip member in it (not this route's), and a
damaged member, which raises OSError."""
import bz2
import filecmp
import gzip
import lzma
import os
import zlib
from os.path import join

import pytest
from click.testing import CliRunner

import dinflate_cases as dc
from helpers import DATA

pytestmark = pytest.mark.gpu

ALN = join(DATA, 'align')
TAX = join(DATA, 'taxonomy')
FUN = join(DATA, 'function')
OUT = join(DATA, 'output')
EOF_BLOCK = dc.bgzf(b'\x03\x00', b'')


def as_bgzf(text, piece=4000, level=6):
    return b''.join(dc.bgzf(dc.raw_deflate(text[i:i + piece], level),
                            text[i:i + piece])
                    for i in range(0, len(text), piece)) + EOF_BLOCK


def classify(params, out, monkeypatch, block=None, off=False):
    """Run the command; returns what ROUTES gained."""
    from woltka_amd.cli import classify_cmd
    from woltka_amd.hostio import ROUTES
    from woltka_amd.routes import device_text
    if block is not None:
        monkeypatch.setattr(device_text.DeviceTextRoute, 'DTOK_BLOCK', block)
    if off:
        monkeypatch.setenv('WOLTKA_NO_DINFLATE', '1')
    else:
        monkeypatch.delenv('WOLTKA_NO_DINFLATE', raising=False)
    before = dict(ROUTES)
    res = CliRunner().invoke(classify_cmd, params + ['--output', out, '--no-exe'],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    return {k: v - before.get(k, 0) for k, v in ROUTES.items()}


def rewrite(src_dir, dst_dir, ext, opener):
    os.makedirs(dst_dir, exist_ok=True)
    for fn in sorted(os.listdir(src_dir)):
        if not fn.endswith(ext):
            continue
        with opener(join(src_dir, fn), 'rb') as f:
            text = f.read()
        with open(join(dst_dir, fn[:-len(ext)] + '.gz'), 'wb') as f:
            f.write(as_bgzf(text))
    return dst_dir


@pytest.fixture(scope='module')
def bowtie2_bgzf(tmp_path_factory):
    return rewrite(join(ALN, 'bowtie2'), str(tmp_path_factory.mktemp('bt2')),
                   '.xz', lzma.open)


@pytest.fixture(scope='module')
def burst_bgzf(tmp_path_factory):
    return rewrite(join(ALN, 'burst'), str(tmp_path_factory.mktemp('burst')),
                   '.bz2', bz2.open)


@pytest.mark.parametrize('block', [1 << 16, 1 << 26])
def test_goldens_as_bgzf(bowtie2_bgzf, tmp_path, monkeypatch, block):
    out = str(tmp_path / 'ogu.tsv')
    got = classify(['--input', bowtie2_bgzf], out, monkeypatch, block)
    print('routes:', got)
    assert filecmp.cmp(out, join(OUT, 'bowtie2.ogu.tsv'), shallow=False)
    assert got.get('dinflate', 0) > 0
    assert got.get('host_block', 0) == 0
    old = str(tmp_path / 'old.tsv')
    got = classify(['--input', bowtie2_bgzf], old, monkeypatch, block, off=True)
    assert filecmp.cmp(old, join(OUT, 'bowtie2.ogu.tsv'), shallow=False)
    assert got.get('dinflate', 0) == 0


@pytest.mark.parametrize('block', [1 << 16, 1 << 26])
def test_goldens_with_coords(bowtie2_bgzf, tmp_path, monkeypatch, block):
    out = str(tmp_path / 'orf.tsv')
    params = ['--input', bowtie2_bgzf, '--coords', join(FUN, 'coords.txt.xz')]
    got = classify(params, out, monkeypatch, block)
    print('routes:', got)
    assert filecmp.cmp(out, join(OUT, 'bowtie2.orf.tsv'), shallow=False)
    assert got.get('dinflate', 0) > 0 and got.get('dhits', 0) > 0
    assert got.get('host_block', 0) == 0
    old = str(tmp_path / 'old.tsv')
    got = classify(params, old, monkeypatch, block, off=True)
    assert filecmp.cmp(old, join(OUT, 'bowtie2.orf.tsv'), shallow=False)
    assert got.get('dinflate', 0) == 0


def test_blast_goldens_as_bgzf(burst_bgzf, tmp_path, monkeypatch):
    out = str(tmp_path / 'genus.tsv')
    got = classify(['--input', burst_bgzf, '--outmap', str(tmp_path / 'maps'),
                    '--names', join(TAX, 'names.dmp'),
                    '--nodes', join(TAX, 'nodes.dmp'),
                    '--map', join(TAX, 'taxid.map'), '--rank', 'genus',
                    '--name-as-id'], out, monkeypatch, 1 << 16)
    print('routes:', got)
    assert filecmp.cmp(out, join(OUT, 'burst.genus.tsv'), shallow=False)
    assert got.get('dinflate', 0) > 0
    for i in range(1, 6):
        with gzip.open(tmp_path / 'maps' / f'S0{i}.txt.gz', 'rt') as f:
            obs = [x.rstrip() for x in f]
        with gzip.open(join(OUT, 'burst.genus.map', f'S0{i}.txt.gz'),
                       'rt') as f:
            exp = [x.rstrip() for x in f]
        assert obs == exp


def records(n, per_query=3, seed=2):
    import random
    rnd = random.Random(seed)
    return b''.join(b'R%09d\t%d\tT%07d\t%d\t42\t50M\t*\t0\t0\t*\t*\n' % (
        i // per_query, rnd.choice((0, 16)), rnd.randrange(300),
        rnd.randrange(1, 10 ** 6)) for i in range(n))


def same_as_plain(text, packed, tmp_path, monkeypatch, block=1 << 16):
    """Tables of `packed` (the text as a .sam.gz) and of the plain text."""
    plain, comp = tmp_path / 'plain', tmp_path / 'comp'
    plain.mkdir()
    comp.mkdir()
    (plain / 'S1.sam').write_bytes(text)
    (comp / 'S1.sam.gz').write_bytes(packed)
    assert gzip.decompress(packed) == text
    a, b = str(tmp_path / 'plain.tsv'), str(tmp_path / 'comp.tsv')
    classify(['--input', str(plain)], a, monkeypatch, block)
    got = classify(['--input', str(comp)], b, monkeypatch, block)
    print('routes:', got)
    assert filecmp.cmp(a, b, shallow=False)
    return got


def test_wk_chain(tmp_path, monkeypatch):
    from woltka_amd import pgzip
    text = records(20000)
    packed = b''.join(pgzip.member(text[i:i + 300000], level=6)
                      for i in range(0, len(text), 300000))
    same_as_plain(text, packed, tmp_path, monkeypatch, 1 << 19)
    # ... and on the device, whose default leaves members this large to the host
    from woltka_amd.routes import device_text
    monkeypatch.setattr(device_text.DeviceTextRoute, 'DINFLATE_MEMBER_MAX', 1 << 30)
    (tmp_path / 'again').mkdir()
    got = same_as_plain(text, packed, tmp_path / 'again', monkeypatch, 1 << 19)
    assert got.get('dinflate', 0) > 0


def test_header_longer_than_the_first_block(tmp_path, monkeypatch):
    head = b'@HD\tVN:1.0\n' + b''.join(
        b'@SQ\tSN:T%07d\tLN:%d\n' % (i, 1000 + i) for i in range(3000))
    assert len(head) > (1 << 16)
    text = head + records(2000)
    got = same_as_plain(text, as_bgzf(text), tmp_path, monkeypatch)
    assert got.get('dinflate', 0) > 0


def test_run_longer_than_a_block(tmp_path, monkeypatch):
    run = b''.join(b'LONGRUN\t0\tT%07d\t%d\t42\t50M\t*\t0\t0\t*\t*\n' % (
        i % 300, i + 1) for i in range(4000))
    assert len(run) > (1 << 16) + (1 << 16)
    text = records(1500) + run + records(1500, seed=3).replace(b'R0', b'Q0')
    got = same_as_plain(text, as_bgzf(text), tmp_path, monkeypatch)
    assert got.get('dinflate', 0) > 0


def test_a_chain_with_an_ordinary_member_goes_the_old_way(tmp_path, monkeypatch):
    text = records(6000)
    packed = as_bgzf(text[:200000])[:-len(EOF_BLOCK)] + gzip.compress(text[200000:])
    got = same_as_plain(text, packed, tmp_path, monkeypatch)
    assert got.get('dinflate', 0) == 0


def test_a_damaged_member_raises(tmp_path, monkeypatch):
    text = records(6000)
    pieces = [text[i:i + 4000] for i in range(0, len(text), 4000)]
    members = [dc.bgzf(dc.raw_deflate(p), p) for p in pieces]
    k = len(members) * 2 // 3
    bad = bytearray(members[k])
    bad[-6] ^= 0x01                     # (its CRC-32)
    members[k] = bytes(bad)
    comp = tmp_path / 'comp'
    comp.mkdir()
    (comp / 'S1.sam.gz').write_bytes(b''.join(members) + EOF_BLOCK)
    with pytest.raises(OSError):
        classify(['--input', str(comp)], str(tmp_path / 'x.tsv'), monkeypatch,
                 1 << 16)
    with pytest.raises(OSError):
        classify(['--input', str(comp)], str(tmp_path / 'y.tsv'), monkeypatch,
                 1 << 16, off=True)
