"""The window limits of the one-kernel SAM tokenizer in 32 bits, on the CPU.

`csrc/wk_dtok_rounds.hpp` gives `fr_min_end(base, len, lim)` for the 64-bit
`min(base + len, lim)` and `fr_fits(base, len, lim)` for `base + len <= lim`
the kernel used to compute with 64-bit sums (a span's end, a window's end, a
wave's round inside the counted text).  The forms are exact for every 32-bit
value -- the argument is written there -- so no block size has to be refused;
the cases the argument rests on lie next to 2^32, where no GPU test can put a
text.  `tests/native/dtok_limits32_host.cpp` -- a program of its own, nothing
is loaded into python -- holds both against the 64-bit arithmetic on every
combination of edge values and on random triples.  It is built with
-fsanitize=address,undefined, as tests/test_dtok_rounds_host.py builds its
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'dtok_limits32_host.cpp')


def test_limits_against_64_bit_arithmetic(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'dtok_limits32_host')
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
