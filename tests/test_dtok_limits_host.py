"""The limit-shape texts of tests/golden/dtok_limits.py on the CPU side (no
GPU): every recipe still makes the text the reference was run on, and the
host tokenizer -- the last fallback of every block the device hands back --
yields what the reference's parser yields on it (tests/golden/vectors/
dtok_limits.json, make_golden.py::gen_dtok_limits), at several thread / block
settings, and refuses where the reference raises."""
import hashlib
import os
import sys

import pytest

from helpers import load_vectors
from test_tokenizer import run_native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                'golden'))
import dtok_limits as D  # noqa: E402

VEC = load_vectors('dtok_limits.json')
NAMES = sorted(D.CASES)


def test_every_case_has_reference_vectors():
    assert sorted(VEC) == NAMES


@pytest.mark.parametrize('name', NAMES)
def test_recipes_make_the_texts_the_reference_read(name):
    """A red GPU test is never a generator that drifted."""
    files, kw = D.case_files(name)
    got = {rel: hashlib.sha256(t.encode()).hexdigest()
           for rel, t in files.items()}
    assert got == VEC[name]['text_sha256']
    assert dict(kw, output_fmt=False) == VEC[name]['kwargs']


# (threads, block bytes): one block, blocks smaller than the lines of
# `long_lines`, blocks of a few lines
SETTINGS = [(1, 1 << 24), (4, 1 << 15), (3, 4093), (2, 977)]


@pytest.mark.parametrize('name', NAMES)
def test_host_tokenizer_yields_what_the_reference_parser_does(name):
    files, kw = D.case_files(name)
    want = VEC[name]['parse']
    excl = set(kw['exclude'].split(',')) if kw.get('exclude') else None
    big = sum(map(len, files.values())) > (4 << 20)
    for threads, block in SETTINGS[:2] if big else SETTINGS:
        for rel in sorted(files):
            text = files[rel].encode()
            if 'error' in want[rel]:
                with pytest.raises(Exception) as e:
                    run_native(text, threads, block, excl=excl)
                assert type(e.value).__name__ == want[rel]['error'], \
                    (rel, threads, block)
                continue
            got, _ = run_native(text, threads, block, excl=excl)
            assert D.parse_digest(got) == want[rel], (rel, threads, block)
