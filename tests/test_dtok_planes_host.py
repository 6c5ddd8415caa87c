"""The plane arithmetic of the one-kernel SAM tokenizer on the CPU.

`csrc/wk_dtok_planes.hpp` gives a record its position and size inside its read
from bit planes of the window's owned lines (run starts; first lines per mate):
the highest run start at or below a line, the lowest above it, population
counts between them.  The functions are plain `__host__ __device__` code, so
`tests/native/dtok_planes_host.cpp` -- a program of its own, nothing is loaded
into python -- holds them against the walks they replace, written out plainly,
on hand-made planes (a head at bit 0 and at bit 63, an end at the next word's
bit 0 and at bit 63, a run over three whole words, 64q and 64q + 1 lines, no
lines, a single-line run at line 1 279, three mate planes of different
patterns) and on random ones of up to 1 280 lines.  It is built with
-fsanitize=address,undefined and planes of exactly the words a case has: a
shift by 64 or a word read past a plane ends it with an error here, not on the
GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'dtok_planes_host.cpp')


def test_planes_against_the_walks(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'dtok_planes_host')
    # (the sanitizers' runtimes inside the program: g++ needs to be told)
    static = ['-static-libasan', '-static-libubsan'] \
        if os.path.basename(cxx).startswith('g++') else []
    subprocess.check_call(
        [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all'] + static + ['-I',
         os.path.join(ROOT, 'woltka_amd', 'csrc'), '-o', exe, SRC])
    res = subprocess.run([exe], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:]
    assert ' 0 failures' in res.stdout
