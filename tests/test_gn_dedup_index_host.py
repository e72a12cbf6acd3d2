"""The index arithmetic of dexct_gn_decompose_dedup (csrc/gn_dedup_index.h) on the host: tests/gn_dedup_index_host.cpp plays census,
scan, gather and expansion on random bit rows for R in {1, 31, 32, 33, 63, 64, 65, 512} and F in {0, 1, 63, 64, 65, cap - 1, cap,
cap + 1}, and checks that the pad range, the queue head and the last entry are consistent, that no index leaves its array or the
workspace, and that the bit / word mapping round-trips.  The program is built twice: plainly, and with the address and
undefined-behaviour sanitizers (it is a stand-alone host program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'gn_dedup_index_host.cpp')
CSRC = os.path.join(ROOT, 'dex-ct-sim_amd', 'csrc')


def _build_and_run(tmp_path, name, extra):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', *extra, '-I', CSRC, SRC, '-o', exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert ' 0 mismatches' in p.stdout, p.stdout[-3000:]
    return p.stdout


def test_gn_dedup_index(tmp_path):
    out = _build_and_run(tmp_path, 'gn_dedup_index_host', [])
    assert int(out.split()[0]) > 100000


def test_gn_dedup_index_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'gn_dedup_index_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
