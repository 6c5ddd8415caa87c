"""The neighbour's verdict of the one-kernel SAM tokenizer on the CPU.

`csrc/wk_dtok_neighbour.hpp` tells whether a mapped line starts a run of equal
QNAMEs from two five-word summaries: the line's own and that of the line
before it, which the kernel takes from the lane below.  A summary carries the
QNAME's length and its first 16 bytes, so the function answers "starts",
"continues" or "undecided" -- and the kernel compares the bytes itself where
it is left undecided.  The functions are plain `__host__ __device__` code, so
`tests/native/dtok_neighbour_host.cpp` -- a program of its own, nothing is
loaded into python -- holds them against a plain compare of whole QNAMEs:
lengths 1, 8, 15, 16, 17 and 40; a difference at byte 0, at byte 15, at byte
16 (undecided, never "continues") and at the last byte; equal first 16 bytes
with different lengths; a predecessor that is unmapped or no line at all
(always undecided); every pair of lengths up to 40 and random names.  The
summaries are made from 16 bytes of a line, what follows the QNAME included.
It is built with -fsanitize=address,undefined: a shift by 64 in the masks
ends it with an error here, not on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'dtok_neighbour_host.cpp')


def test_verdict_against_whole_qnames(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'dtok_neighbour_host')
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
