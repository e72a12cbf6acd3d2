"""The gather's batch arithmetic of dexct_gn_decompose_dedup (csrc/gn_dedup_index.h: gather_batch_lines, gather_batches,
word_of_fresh, select_bit, pixel_of_batch_word) on the host: tests/gn_dedup_gather_index_host.cpp plays the gather batch by batch
and chunk by chunk on random bit rows - rows with one to eight words and a partial last word, a line with exactly and with more
than a chunk's words, line counts one below, at and one above a multiple of the batch, lines without a fresh pixel after row 0 and
lines fresh in every row - and checks that every fresh pixel is moved once, in the order of the pixels, to consecutive places, and
that no index leaves its array.  The program is built twice: plainly, and with the address and undefined-behaviour sanitizers
(it is a stand-alone host program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'gn_dedup_gather_index_host.cpp')
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


def test_gn_dedup_gather_index(tmp_path):
    out = _build_and_run(tmp_path, 'gn_dedup_gather_index_host', [])
    assert int(out.split()[0]) > 100000


def test_gn_dedup_gather_index_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'gn_dedup_gather_index_host_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
