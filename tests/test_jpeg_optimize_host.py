"""CPU tests of the host half of the encoder's optimised Huffman coding: frp_jpeg_optimal_table (needs only the built library, no GPU)
against the model's gen_optimal_table (tests/jpeg_optimize_model.py, which tests/test_jpeg_optimize_model.py pins to Pillow's files),
its refusals, and the flag's value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_encode_model as M
import jpeg_optimize_model as OM
from frp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = OM.cases()


def _tables_of(hist):
    """the four count tables of a histogram, each widened to 256 entries: DC0, AC0, DC1, AC1"""
    out = []
    for t in (0, 1):
        dc = np.zeros(256, np.uint32)
        dc[:16] = hist[16 * t:16 * t + 16]
        out += [dc, hist[OM.AC0 + 256 * t:OM.AC0 + 256 * (t + 1)]]
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_image_histograms_give_the_model_s_tables(name):
    rgb, q, ss, r = CASES[name]
    info, coef, _ = M.forward(rgb, q, ss)
    hist = OM.histogram(info, coef, r)
    for k, freq in enumerate(_tables_of(hist)):
        bits, vals = native.jpeg_optimal_table(freq)
        assert (bits, vals) == OM.gen_optimal_table(freq), (name, k)
        assert max(i + 1 for i in range(16) if bits[i]) <= 16


def test_tie_heavy_counts_equal_the_model():
    """the library picks the two least frequent entries from a heap, the model by libjpeg's two linear searches: counts full of ties
    (0..3, all ones, powers of two) are where the two could part"""
    rng = np.random.default_rng(99)
    for it in range(60):
        freq = np.zeros(256, np.uint32)
        idx = rng.permutation(256)[:int(rng.integers(1, 65))]
        kind = it % 3
        freq[idx] = rng.integers(0, 4, size=idx.size) if kind == 0 else 1 if kind == 1 else 1 << rng.integers(0, 12, size=idx.size)
        if not freq.any():
            freq[idx[0]] = 1
        assert native.jpeg_optimal_table(freq) == OM.gen_optimal_table(freq), it


def _fibonacci(n_symbols, seed):
    """Fibonacci counts 1, 2, 3, 5, ... on n_symbols of the 256 indices, scattered: with the pseudo-symbol's 1 in front the sequence is
    1, 1, 2, 3, 5, ..., whose unlimited Huffman code is a comb, as deep as there are symbols"""
    fib = [1, 2]
    while len(fib) < n_symbols:
        fib.append(fib[-1] + fib[-2])
    idx = np.random.default_rng(seed).permutation(256)[:n_symbols]
    freq = np.zeros(256, np.uint32)
    freq[idx] = fib
    return freq


@pytest.mark.parametrize("n_symbols", [20, 25])
def test_the_length_limiting_branch(n_symbols):
    """Counts whose unlimited code is deeper than 16, so Figure K.3's adjustment runs.  No image tried while this was written (up to
    640 x 480) got past length 16 before limiting, so Pillow never showed this branch: it is held to the model and to its
    invariants only - every length <= 16, the Kraft sum with the pseudo-symbol's code <= 1, the symbol count preserved, vals ordered
    by code length (of the unlimited code) and then by value."""
    freq = _fibonacci(n_symbols, n_symbols)
    assert freq.max() < 2 ** 31 and np.count_nonzero(freq) == n_symbols
    bits, vals = native.jpeg_optimal_table(freq)
    assert (bits, vals) == OM.gen_optimal_table(freq)
    depth = {s: d for s, d in enumerate(OM.code_sizes(freq)[:256]) if d}      # before limiting: deeper than 16, within libjpeg's 32
    assert 16 < max(depth.values()) <= 32
    assert len(bits) == 16 and sum(bits) == len(vals) == n_symbols
    assert sorted(vals) == np.flatnonzero(freq).tolist()
    longest = max(i + 1 for i in range(16) if bits[i])
    assert sum(b * 2 ** (16 - (i + 1)) for i, b in enumerate(bits)) + 2 ** (16 - longest) <= 2 ** 16
    assert vals == sorted(vals, key=lambda s: (depth[s], s))
    # more frequent symbols never get longer codes
    length = {}
    k = 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            length[vals[k]] = ln
            k += 1
    order = sorted(vals, key=lambda s: -int(freq[s]))
    assert all(length[a] <= length[b] for a, b in zip(order, order[1:]) if freq[a] > freq[b])


def test_refusals_and_the_smallest_table():
    lib = native.load_library()
    bits, vals = np.full(16, 0xA5, np.uint8), np.full(256, 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # Fibonacci over 36 symbols: deeper than 32 bits before limiting, where libjpeg gives up
    deep = _fibonacci(36, 36)
    assert lib.frp_jpeg_optimal_table(p(deep), p(bits), p(vals)) == -1
    with pytest.raises(ValueError):
        OM.gen_optimal_table(deep)
    zero = np.zeros(256, np.uint32)
    assert lib.frp_jpeg_optimal_table(p(zero), p(bits), p(vals)) == -1
    assert lib.frp_jpeg_optimal_table(None, p(bits), p(vals)) == -1
    assert lib.frp_jpeg_optimal_table(p(deep), None, p(vals)) == -1 and lib.frp_jpeg_optimal_table(p(deep), p(bits), None) == -1
    assert (bits == 0xA5).all() and (vals == 0xA5).all()      # nothing written
    for bad in (deep, zero):
        with pytest.raises(native.FrpError):
            native.jpeg_optimal_table(bad)
    with pytest.raises(ValueError):
        native.jpeg_optimal_table(np.zeros(255, np.uint32))
    # one symbol: a 1-bit code
    one = np.zeros(256, np.uint32)
    one[0xF0] = 4_000_000_000                                 # (and a count near the top of uint32)
    assert lib.frp_jpeg_optimal_table(p(one), p(bits), p(vals)) == 1
    assert bits.tolist() == [1] + [0] * 15 and vals[0] == 0xF0 and (vals[1:] == 0xA5).all()
    assert native.jpeg_optimal_table(one) == ([1] + [0] * 15, [0xF0])


def test_flag_and_symbols():
    header = open(os.path.join(ROOT, "include", "frp.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (FRP_FLAG_\w+) (\d+)u", header)}
    assert flags["FRP_FLAG_JPEG_OPTIMIZE"] == native.FLAG_JPEG_OPTIMIZE
    assert list(flags.values()).count(native.FLAG_JPEG_OPTIMIZE) == 1
    assert native.FLAG_JPEG_OPTIMIZE == min(1 << b for b in range(32) if (1 << b) not in set(flags.values()) - {native.FLAG_JPEG_OPTIMIZE})
    assert native.FLAG_JPEG_OPTIMIZE not in (1, 4, 1 << 31)
    assert int(re.search(r"#define FRP_JPEG_HIST_ELEMS (\d+)", header).group(1)) == native.JPEG_HIST_ELEMS == OM.HIST_ELEMS
    lib = native.load_library()
    for name in ("frp_jpeg_optimal_table", "frp_encode_jpeg_histograms"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
