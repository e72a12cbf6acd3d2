"""The tile rule on the host (csrc/tile_class.h: the tile map's layout and builder rule, the rule that dismisses a run of slabs, the
sharing-out of runs and fine slabs to lanes and the bound on the per-lane count; csrc/proj_pure.h: proj::use_tile_map):
tests/tile_class_host.cpp, a brute force over small grids against the slab rule, built twice - plainly, and with the address and
undefined-behaviour sanitizers (it is a stand-alone host program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'tile_class_host.cpp')
CSRC = os.path.join(ROOT, 'dex-ct-sim_amd', 'csrc')


def _build_and_run(tmp_path, name, extra):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', *extra, '-I', CSRC, SRC, '-o', exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert ' 0 mismatches' in p.stdout, p.stdout[-3000:]
    return p.stdout


def test_tile_rule_against_the_slab_rule(tmp_path):
    out = _build_and_run(tmp_path, 'tile_class_host', [])
    assert int(out.split()[0]) > 100000


def test_tile_rule_against_the_slab_rule_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'tile_class_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
