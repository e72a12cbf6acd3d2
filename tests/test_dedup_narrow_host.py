"""The narrow list rounds of rows16_kernel on the host (csrc/dedup_index.h: the rows per lane of a round, the entry and the rows a
lane detects, the pieces of the entry it reads and writes): tests/dedup_narrow_host.cpp, built twice - plainly, and with the
address and undefined-behaviour sanitizers (it is a stand-alone host program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'dedup_narrow_host.cpp')
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


def test_every_row_of_every_entry_once_and_inside_its_entry(tmp_path):
    out = _build_and_run(tmp_path, 'dedup_narrow_host', [])
    assert int(out.split()[0]) > 100000


def test_every_row_of_every_entry_once_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'dedup_narrow_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
