"""The device DEFLATE encoder's parts that need no device: the code-length
routine the kernel runs (deflate_codes.h through bqsr_deflate_code_lengths),
the member routine compiled for the host (bqsr_bgzf_deflate_host: the same
source as the kernel, a lane at a time) against zlib as the decoder, and the
command line's refusals around -bam_compressor."""
import heapq

import numpy as np
import pytest

import _deflate_cases as C
from adam_amd import _capi
from adam_amd.sam import bgzf_deflate_host, deflate_code_lengths
from adam_amd.transform import main, transform

SHAPES = [(286, 15), (30, 15), (19, 7)]


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def huffman_depths(freq):
    """{symbol: depth} of a heapq Huffman tree over the used symbols (>= 2)"""
    heap = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    depth = {s: 0 for _, _, (s,) in heap}
    heapq.heapify(heap)
    tie = len(freq)
    while len(heap) > 1:
        fa, _, sa = heapq.heappop(heap)
        fb, _, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, tie, sa + sb))
        tie += 1
    return depth


def histograms(n_syms, max_bits):
    rng = np.random.default_rng(1000 * n_syms + max_bits)
    k = 22 if max_bits == 15 else 10  # unrestricted depth 21 / 9: above max_bits
    h = {"fibonacci": np.array(fib(k) + [0] * (n_syms - k)),
         "fibonacci_scattered": np.zeros(n_syms, np.int64),
         "all_zero": np.zeros(n_syms, np.int64),
         "one": np.zeros(n_syms, np.int64),
         "two": np.zeros(n_syms, np.int64),
         "all_equal": np.full(n_syms, 7),
         "random": rng.integers(0, 1000, n_syms),
         "random_sparse": rng.integers(0, 50, n_syms) * (rng.random(n_syms) < 0.3),
         "random_skewed": (rng.pareto(0.7, n_syms) * 3).astype(np.int64)}
    h["fibonacci_scattered"][rng.permutation(n_syms)[:k]] = fib(k)
    h["one"][n_syms // 2] = 5
    h["two"][[1, n_syms - 1]] = [3, 100000]
    return h


@pytest.mark.parametrize("n_syms,max_bits", SHAPES)
def test_code_lengths(n_syms, max_bits):
    assert huffman_depths(fib(22))[0] == 21 and huffman_depths(fib(10))[0] == 9
    for name, freq in histograms(n_syms, max_bits).items():
        freq = np.asarray(freq, np.int64)
        lens = deflate_code_lengths(freq, max_bits).astype(np.int64)
        used = freq > 0
        assert lens.shape == (n_syms,), name
        assert (lens[~used] == 0).all(), name
        assert ((lens[used] >= 1) & (lens[used] <= max_bits)).all(), name
        if used.sum() == 1:
            assert lens[used][0] == 1, name
        if used.sum() >= 2:  # Kraft sum exactly 1, in integers
            assert int((2 ** (max_bits - lens[used])).sum()) == 2 ** max_bits, name
            depth = huffman_depths(freq.tolist())
            if max(depth.values()) <= max_bits:  # the plain Huffman code fits: its cost
                assert int((freq * lens).sum()) == sum(int(freq[s]) * d for s, d in depth.items()), name
            else:  # limited: no cheaper than the optimum
                assert int((freq * lens).sum()) >= sum(int(freq[s]) * d for s, d in depth.items()), name


def test_fibonacci_is_limited():
    """the two histograms the limit exists for: depth 21 at 15 bits, 9 at 7"""
    for k, n_syms, max_bits in ((22, 286, 15), (22, 30, 15), (10, 19, 7)):
        lens = deflate_code_lengths(fib(k) + [0] * (n_syms - k), max_bits)
        assert lens[:k].max() == max_bits and lens[k:].max(initial=0) == 0
        assert sum(2 ** (max_bits - int(l)) for l in lens[:k]) == 2 ** max_bits
        assert all(lens[i] >= lens[i + 1] for i in range(1, k - 1))  # rarer symbols never get shorter codes


def test_more_symbols_than_codes_is_refused():
    for n_syms, max_bits in ((129, 7), (20, 4), (5, 0), (5, 16)):
        with pytest.raises(_capi.BQSRError) as e:
            deflate_code_lengths(np.ones(n_syms), max_bits)
        assert e.value.status == _capi.INVALID_ARG
    assert (deflate_code_lengths(np.ones(128), 7) == 7).all()


# ---- the member routine on the host: the kernel's source, a lane at a time ----

@pytest.mark.parametrize("n", C.SIZES)
def test_host_routine_sizes(n):
    for data in (C.random_bytes(n, n), bytes(n)):
        out = bgzf_deflate_host(data)
        C.check_members(out, data)
        assert out == bgzf_deflate_host(data)


@pytest.mark.parametrize("name", C.CONTENTS)
def test_host_routine_contents(name):
    data = C.content(name)
    ms = C.check_members(bgzf_deflate_host(data), data)
    C.check_sizes(name, ms)


def test_host_routine_small_output_is_reported():
    import ctypes
    from adam_amd.sam import _lib
    data = np.frombuffer(C.content("A"), np.uint8)
    want = len(bgzf_deflate_host(data))
    out = np.zeros(want, np.uint8)
    got = ctypes.c_int64()
    L = _lib()
    assert L.bqsr_bgzf_deflate_host(data.ctypes.data, data.size, out.ctypes.data, want - 1, ctypes.byref(got),
                                    None) == _capi.INVALID_ARG
    assert got.value == want
    assert L.bqsr_bgzf_deflate_host(data.ctypes.data, data.size, out.ctypes.data, want, ctypes.byref(got), None) == 0
    C.check_members(out.tobytes(), data.tobytes())


# ---- the command line ----

def test_device_compressor_with_a_level_is_refused(tmp_path, capsys):
    inp, out = str(tmp_path / "in.sam"), str(tmp_path / "X.bam")
    with open(inp, "wb") as fh:
        fh.write(b"@HD\tVN:1.4\n")
    with pytest.raises(SystemExit) as e:
        main([inp, out, "-bam_compressor", "device", "-bam_compression_level", "6"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "one level" in err and "-bam_compression_level" in err
    with pytest.raises(ValueError, match="one level"):
        transform(inp, out, bam_compressor="device", bam_level=1)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.sam"]


@pytest.mark.parametrize("which", ["host", "device"])
def test_compressor_with_another_output_is_refused(tmp_path, capsys, which):
    inp = str(tmp_path / "in.sam")
    with open(inp, "wb") as fh:
        fh.write(b"@HD\tVN:1.4\n")
    for out in ("X.sam", "X.adam"):
        with pytest.raises(SystemExit) as e:
            main([inp, str(tmp_path / out), "-bam_compressor", which])
        assert e.value.code == 2
        assert "BAM output only" in capsys.readouterr().err
        with pytest.raises(ValueError, match="BAM output only"):
            transform(inp, str(tmp_path / out), bam_compressor=which)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.sam"]


def test_unknown_compressor_is_refused(tmp_path, capsys):
    with pytest.raises(SystemExit):
        main([str(tmp_path / "in.sam"), str(tmp_path / "X.bam"), "-bam_compressor", "zstd"])
    assert "-bam_compressor" in capsys.readouterr().err
    with pytest.raises(ValueError, match="-bam_compressor"):
        transform(str(tmp_path / "in.sam"), str(tmp_path / "X.bam"), bam_compressor="zstd")
