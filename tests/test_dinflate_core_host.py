"""The device inflater's core on the CPU, under AddressSanitizer.

`csrc/wk_dinflate_core.hpp` holds everything of the device inflater that
decides bytes, as plain `__host__ __device__` functions over an `Io` that owns
the storage.  `tests/native/dinflate_core_host.cpp` -- a program of its own,
nothing is loaded into python -- runs them over the chains of
`tests/dinflate_cases.py`: every member is decoded from a heap copy of
exactly its compressed span into a heap buffer of exactly its stated size,
so an access outside a member's spans ends the program, whether the stream is
one zlib wrote, one assembled bit by bit (distance 32 768, codes of 15 bits,
one or no distance code, 5 and 13 extra bits) or a damaged one, whose status
is pinned.  The expected bytes are zlib's.  The CRC is folded as the kernel
folds it (64 lane states over runs of 2 KB) and, cut into pieces of 0, 1, 63,
64, 65 and 65 280 bytes, held against `zlib.crc32`."""
import os
import shutil
import subprocess

import pytest

import dinflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'dinflate_core_host.cpp')


def test_core_inside_its_spans(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++ or clang++) to build ' + SRC)
    exe = str(tmp_path / 'dinflate_core_host')
    # (the sanitizers' runtimes inside the program: g++ needs to be told)
    static = ['-static-libasan', '-static-libubsan'] \
        if os.path.basename(cxx).startswith('g++') else []
    subprocess.check_call(
        [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all'] + static + ['-I',
         os.path.join(ROOT, 'woltka_amd', 'csrc'), '-o', exe, SRC])
    cases = dc.good_cases() + dc.damage_cases()
    path = str(tmp_path / 'cases.bin')
    dc.write_file(path, cases, dc.crc_cases())
    res = subprocess.run([exe, path], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:]
    assert '%d cases' % len(cases) in res.stdout
    assert ' 0 failures' in res.stdout
