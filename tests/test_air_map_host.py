"""The pure decisions of the projection host layer (csrc/proj_pure.h) on the host: tests/air_map_host.cpp drives
proj::use_air_map - whether a launch of rows16_kernel looks columns up in the air-column map - through every mode, a missing
map, impossible counts and the share of air columns at its boundary.  The program is built twice: plainly, and with the address
and undefined-behaviour sanitizers (it is a stand-alone host program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'air_map_host.cpp')
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


def test_use_air_map(tmp_path):
    out = _build_and_run(tmp_path, 'air_map_host', [])
    assert int(out.split()[0]) > 400


def test_use_air_map_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'air_map_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
