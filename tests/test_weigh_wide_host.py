"""The bucket and work-list arithmetic of the wide weighted histogram on the
CPU.

`csrc/wk_weigh_wide.hpp` says which bucket a packed word belongs to
(`wide_bucket`, with the clamp into the last bucket) and, from the buckets'
counts, where every bucket's records lie in the second buffer and which items
-- a team's share of one bucket, one slab row -- the histogram's workgroups
walk (`wide_plan`, run by one thread of the scan kernel).  Both are plain
`__host__ __device__` code, so `tests/native/weigh_wide_host.cpp` -- a program
of its own, nothing is loaded into python -- holds them against plain
arithmetic: seams and the clamp, empty tables, one record, 207 buckets of one
record, all records in one bucket at the largest count a flush holds, Zipf
counts with the head first and last, random counts, for 1 to 1 024
workgroups.  It is built with -fsanitize=address,undefined, as
tests/test_dtok_rounds_host.py builds its program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'weigh_wide_host.cpp')


def test_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'weigh_wide_host')
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
