"""The dealing of the one-kernel SAM tokenizer's line pass on the CPU.

`csrc/wk_dtok_neighbour.hpp` deals a window's lines so that the line before a
lane's line is the lane below's inside one wave: lanes 1..63 own 63 consecutive
lines, lane 0 is the witness of the line in front of them (the last own line
of the wave before, or of thread 511's wave in the trip before) and owns
nothing; a trip of eight waves covers 504 lines.  The functions are plain
`__host__ __device__` code, so `tests/native/dtok_witness_host.cpp` -- a
program of its own, nothing is loaded into python -- runs the kernel's loop
for 1, 62, 63, 64, 503, 504, 505, 1 008 and 1 023 lines with `first_line` 0 and
1 and holds it against plain enumeration: every line has exactly one owning
lane; every owner's lane below holds the line before, or "no line" for the
window's first line only; no witness owns a line; the trip count is
ceil(lines / 504).  It is built with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'dtok_witness_host.cpp')


def test_dealing_against_enumeration(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'dtok_witness_host')
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
    assert ' 18 cases, 0 failures' in res.stdout
