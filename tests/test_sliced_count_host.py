"""The bit-sliced counters of rows16_kernel (csrc/sliced_count.h) on the host: tests/sliced_count_host.cpp includes the
header with its portable adders, drives word streams (random, sparse, all-ones, all-zero, alternating, one bit position;
0 .. 2047 words) through add16 / add8 / add4 in mixed order and compares every one of the 32 counters with the plain
per-bit count; one stream takes every counter to 2047, all 11 planes set.  The program is built twice: plainly, and
with the address and undefined-behaviour sanitizers (it is a stand-alone host program)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'sliced_count_host.cpp')
CSRC = os.path.join(ROOT, 'dex-ct-sim_amd', 'csrc')


def _build_and_run(tmp_path, name, extra):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Wno-unknown-pragmas', *extra, '-I', CSRC, SRC, '-o', exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert ' 0 mismatches' in p.stdout, p.stdout[-3000:]
    return p.stdout


def test_sliced_counters_equal_plain_counts(tmp_path):
    out = _build_and_run(tmp_path, 'sliced_count_host', [])
    assert int(out.split()[0]) > 800          # 7 schedules x 12 lengths x 10 streams + the full counters


def test_sliced_counters_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'sliced_count_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
