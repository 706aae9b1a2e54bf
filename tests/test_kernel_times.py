"""The eight ``bqsr_*_kernel_times`` calls and their Python wrappers without a
device: the symbols are exported and listed, a thread that ran no job reads
zeros, each call handles a null as the header says, every module's wrapper
gives its KERNELS, and _capi.bind applies a module's table once, for that
module alone."""
import ctypes
import os
import subprocess
import sys
import threading

import pytest

from adam_amd import _capi, aggregate_pileups as AP
from adam_amd import compare as C
from adam_amd import mpileup as M
from adam_amd import print_tags as PT
from adam_amd import reads2ref as R
from adam_amd import realignment_targets as RT
from adam_amd import sam as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# export -> (stages, takes one array, takes a leading handle)
CALLS = {
    "bqsr_pileup_kernel_times": (2, False, False),
    "bqsr_mpileup_kernel_times": (5, True, False),
    "bqsr_realign_targets_kernel_times": (7, True, False),
    "bqsr_pileup_agg_kernel_times": (4, False, False),
    "bqsr_bam_kernel_times": (2, False, False),
    "bqsr_bgzf_deflate_times": (2, False, False),
    "bqsr_tags_kernel_times": (2, False, False),
    "bqsr_compare_kernel_times": (3, False, True),
}
# the wrappers over the thread's values: (call, its stage names, returns a dict)
WRAPPERS = [(R.kernel_times, R.KERNELS, False), (M.kernel_times, M.KERNELS, True), (RT.kernel_times, RT.KERNELS, True),
            (AP.kernel_times, AP.KERNELS, True), (S.bam_kernel_times, S.BAM_KERNELS, False),
            (S.bgzf_deflate_times, S.DEFLATE_KERNELS, False), (PT.kernel_times, PT.KERNELS, False)]


def raw():
    """the library loaded afresh: no module's table has touched its functions"""
    L = ctypes.CDLL(_capi.LIB_PATH)
    dp = ctypes.POINTER(ctypes.c_double)
    for name, (n, array, handle) in CALLS.items():
        f = getattr(L, name)
        f.restype = ctypes.c_int
        f.argtypes = ([ctypes.c_void_p] if handle else []) + ([dp] if array else [dp] * n)
    return L


def on_a_fresh_thread(call):
    out = []
    t = threading.Thread(target=lambda: out.append(call()))
    t.start()
    t.join()
    return out[0]


def test_the_eight_calls_are_listed_and_exported():
    assert set(CALLS) <= set(_capi.EXPORTS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in CALLS)
    assert sorted(n for n in _capi.EXPORTS if n.endswith("_times") and n != "bqsr_batch_layout_times") == sorted(CALLS)


@pytest.mark.parametrize("name", sorted(set(CALLS) - {"bqsr_compare_kernel_times"}))
def test_a_fresh_thread_reads_zeros(name):
    n, array, _ = CALLS[name]
    L = raw()

    def read():
        v = (ctypes.c_double * n)(*([-1.0] * n))
        at = ctypes.addressof(v)
        args = [v] if array else [ctypes.cast(at + 8 * i, ctypes.POINTER(ctypes.c_double)) for i in range(n)]
        assert getattr(L, name)(*args) == _capi.BQSR_OK
        return list(v)

    assert on_a_fresh_thread(read) == [0.0] * n


def test_null_handling():
    L = raw()
    bad = _capi.INVALID_ARG
    # mpileup and realignment targets fill one array and refuse a null one
    assert L.bqsr_mpileup_kernel_times(None) == bad
    assert L.bqsr_realign_targets_kernel_times(None) == bad
    # compare refuses a null handle (its times are the handle's)
    d = ctypes.c_double(-1.0)
    assert L.bqsr_compare_kernel_times(None, ctypes.byref(d), None, None) == bad and d.value == -1.0
    # the others skip a null pointer and fill the rest
    for name in ("bqsr_pileup_kernel_times", "bqsr_pileup_agg_kernel_times", "bqsr_bam_kernel_times",
                 "bqsr_bgzf_deflate_times", "bqsr_tags_kernel_times"):
        n = CALLS[name][0]
        f = getattr(L, name)

        def skip(k):
            v = [ctypes.c_double(-1.0) for _ in range(n)]
            assert f(*[None if i == k else ctypes.byref(x) for i, x in enumerate(v)]) == _capi.BQSR_OK
            return [x.value for x in v]

        assert f(*([None] * n)) == _capi.BQSR_OK
        for k in range(n):
            got = on_a_fresh_thread(lambda: skip(k))
            assert got == [-1.0 if i == k else 0.0 for i in range(n)], (name, k)


def test_wrappers_give_their_kernels_in_order():
    for call, names, is_dict in WRAPPERS:
        got = on_a_fresh_thread(call)
        assert len(names) == len(set(names)) == len(got)
        if is_dict:
            assert list(got) == list(names) and list(got.values()) == [0.0] * len(names)
        else:
            assert isinstance(got, tuple) and got == (0.0,) * len(names)
    assert C.KERNELS == ("join", "scalar", "baseqs")
    assert M.KERNELS == ("walk", "emit", "sort", "group", "text")
    assert RT.KERNELS == ("count", "emit", "sort", "rods", "candidates", "fold_host", "sets")
    assert AP.KERNELS == ("keys", "sort", "scans", "emit")


def test_stage_times_takes_pointers_or_an_array_and_a_handle():
    names = ("a", "b", "c")
    want = {"a": 1.0, "b": 2.0, "c": 3.0}
    seen = []

    def by_pointers(*args):
        seen.append(args[:-3])
        for i, p in enumerate(args[-3:]):
            p[0] = i + 1.0
        return _capi.BQSR_OK

    def by_array(a):
        for i in range(3):
            a[i] = i + 1.0
        return _capi.BQSR_OK

    assert _capi.stage_times(by_pointers, names) == want and seen[-1] == ()
    assert _capi.stage_times(by_pointers, names, handle=7) == want and seen[-1] == (7,)
    assert list(_capi.stage_times(by_array, names, array=True).items()) == list(want.items())
    with pytest.raises(_capi.BQSRError):
        _capi.stage_times(lambda *a: _capi.INVALID_ARG, names)


def test_bind_twice_is_harmless():
    L = ctypes.CDLL(_capi.LIB_PATH)
    sig = {"bqsr_mpileup_kernel_times": (ctypes.c_int, [_capi.dblp]), "bqsr_sam_destroy": (None, [_capi.vp])}
    assert _capi.bind(L, sig) is L
    f = L.bqsr_mpileup_kernel_times
    assert f.restype is ctypes.c_int and list(f.argtypes) == [_capi.dblp] and L.bqsr_sam_destroy.restype is None
    assert _capi.bind(L, sig) is L
    assert L.bqsr_mpileup_kernel_times is f and list(f.argtypes) == [_capi.dblp]
    assert f(None) == _capi.INVALID_ARG
    # a module's _lib() is the same library however often it is asked for
    assert M._lib() is M._lib() is _capi.lib()
    assert list(M._lib().bqsr_mpileup_kernel_times.argtypes) == [_capi.dblp]


CHILD = """
import ctypes, sys
sys.path.insert(0, %r)
from adam_amd import _capi
from adam_amd import mpileup as M
assert "adam_amd.reads2ref" not in sys.modules, "mpileup imports reads2ref before it needs it"
L = M._lib()
for name, (res, args) in M._SIG.items():
    f = getattr(L, name)
    assert f.restype is res and list(f.argtypes) == list(args), name
assert L.bqsr_sam_pileup_prepare.argtypes is None, "mpileup bound reads2ref's table"
assert "adam_amd.reads2ref" not in sys.modules
assert L.bqsr_mpileup_kernel_times(None) == _capi.INVALID_ARG
assert M.kernel_times() == dict.fromkeys(M.KERNELS, 0.0)
print("mpileup alone: ok")
"""


def test_mpileup_binds_its_own_symbols_alone():
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "mpileup alone: ok"
