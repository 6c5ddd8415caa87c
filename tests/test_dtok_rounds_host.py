"""The dealing of a window's chunks in the one-kernel SAM tokenizer on the CPU.

`csrc/wk_dtok_rounds.hpp` says which 16-byte chunks of a window a wave takes
(waves 0-3 three full rounds of 64, waves 4-7 two) and packs a wave's newline
counts, round by round, into the fields of one word.  The functions are plain
`__host__ __device__` code, so `tests/native/dtok_rounds_host.cpp` -- a
program of its own, nothing is loaded into python -- checks that the dealing
covers chunks 0 to 1 280 once each and in order, that packing and unpacking
round-trip at 0, 1, 8 x 64 and the largest count of a kept window (next to
full neighbouring fields), and that the kernel's way to a window's newlines
and to every chunk's first line number equals a plain count on hand-made
(the waves' seams) and random masks, chunks of more than eight newlines
included: those are dropped and reported.  It is built with
-fsanitize=address,undefined, as tests/test_dtok_planes_host.py builds its
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'dtok_rounds_host.cpp')


def test_rounds_against_a_plain_count(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'dtok_rounds_host')
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
