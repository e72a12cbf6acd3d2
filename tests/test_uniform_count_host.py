"""What the column-class map adds on the host (csrc/proj_pure.h: proj::class_counts_ok, proj::use_class_map; csrc/uniform_count.h:
the lookup in either kind of column map, the rule that lets a slab leave rows16_kernel's lists and the packed per-lane count of the
slabs that left): tests/uniform_count_host.cpp, built twice - plainly, and with the address and undefined-behaviour sanitizers (it
is a stand-alone host program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'uniform_count_host.cpp')
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


def test_class_map_rule_lookup_and_counts(tmp_path):
    out = _build_and_run(tmp_path, 'uniform_count_host', [])
    assert int(out.split()[0]) > 10000


def test_class_map_rule_lookup_and_counts_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'uniform_count_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
