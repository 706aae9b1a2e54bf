"""The realignment-target calls of the C ABI without a device: the symbols are
exported and listed, the ctypes mirrors of adam_amd/realignment_targets.py
match the header's structures field for field (names from the header's text,
sizes and offsets from a compiler), and the argument checks answer before any
device call."""
import ctypes
import os
import shutil
import subprocess

from adam_amd import _capi
from adam_amd import realignment_targets as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRRORS = {
    "bqsr_realign_targets_sizes": RT.RealignTargetsSizes,
    "bqsr_realign_targets_host": RT.RealignTargetsHost,
}
SYMBOLS = {"bqsr_sam_realign_targets_prepare", "bqsr_sam_realign_targets_fetch", "bqsr_arrow_realign_targets_prepare",
           "bqsr_arrow_realign_targets_fetch", "bqsr_realign_targets_kernel_times"}


def header_fields(name):
    with open(os.path.join(ROOT, "include", "adam_sam.h")) as fh:
        text = fh.read()
    body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
    return [l.split(";")[0].split()[-1].lstrip("*") for l in body.splitlines()[1:] if ";" in l]


def test_new_symbols_are_listed():
    assert SYMBOLS <= set(_capi.EXPORTS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in SYMBOLS)
    assert len(_capi.STATUS_NAMES) == 17  # no status code was added


def test_field_order_matches_the_header():
    for name, cls in MIRRORS.items():
        assert header_fields(name) == [f for f, _ in cls._fields_], name
    assert tuple(header_fields("bqsr_realign_targets_host")) == RT.COLUMNS


def test_layouts_match_the_compiler(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = ['#include <cstddef>', '#include <cstdio>', '#include "adam_sam.h"', 'int main() {']
    for name in MIRRORS:
        src.append('  std::printf("layout %s %%zu", sizeof(%s));' % (name, name))
        for f in header_fields(name):
            src.append('  std::printf(" %%zu", offsetof(%s, %s));' % (name, f))
        src.append('  std::printf("\\n");')
    src += ['  return 0;', '}']
    path = str(tmp_path / "layout.cpp")
    with open(path, "w") as fh:
        fh.write("\n".join(src) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), path, "-o", exe],
                   check=True)
    seen = {}
    for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        f = l.split()
        seen[f[1]] = [int(x) for x in f[2:]]
    assert set(seen) == set(MIRRORS)
    for name, cls in MIRRORS.items():
        assert seen[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name


def test_argument_checks_without_a_device():
    L = RT._lib()
    sz = RT.RealignTargetsSizes()
    H = RT.RealignTargetsHost()
    fake = ctypes.c_void_p(8)  # never dereferenced: the other argument is null
    bad = _capi.INVALID_ARG
    for prepare in (L.bqsr_sam_realign_targets_prepare, L.bqsr_arrow_realign_targets_prepare):
        assert prepare(None, fake, None, ctypes.byref(sz)) == bad
        assert prepare(fake, None, None, ctypes.byref(sz)) == bad
        assert prepare(fake, fake, None, None) == bad
        assert b"realign_targets_prepare: bad arguments" in L.bqsr_last_error()
    for fetch in (L.bqsr_sam_realign_targets_fetch, L.bqsr_arrow_realign_targets_fetch):
        assert fetch(None, fake, ctypes.byref(H), None) == bad
        assert fetch(fake, None, ctypes.byref(H), None) == bad
        assert fetch(fake, fake, None, None) == bad
        assert b"realign_targets_fetch: bad arguments" in L.bqsr_last_error()
    assert L.bqsr_realign_targets_kernel_times(None) == bad
    ms = (ctypes.c_double * 7)(*([-1.0] * 7))
    assert L.bqsr_realign_targets_kernel_times(ms) == 0
    assert all(v >= 0.0 for v in ms)  # (all 0 unless a prepare ran on this thread)
    assert list(RT.kernel_times()) == list(RT.KERNELS)
