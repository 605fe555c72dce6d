"""The pieces of a random draw on the device, bit for bit.

The device build of af_math.hpp forms Philox's `hi ^ c ^ key` with one three-input bit operation, divides `f / (2 + f)` in
af_log_unit without the scale / fix-up instructions of the IEEE sequence, and makes `a x 2^26 + b` and `1 - K x 2^-53` one fma
each.  The host build of the same header (tests/hostcheck), the oracle (oracle/des_oracle.c) and numpy's IEEE arithmetic keep
the plain text: every device result below must have their bits."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

SQRT_HALF_HI = 0x3FE6A09E      # af_log_unit reduces x to [bits 0x3fe6a09e00000000, that + 2^52)


def _f64(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def _log_unit_inputs() -> np.ndarray:
    named = [1.0, 1.0 - 2.0 ** -53, 2.0 ** -53, 1e-15]
    powers = [2.0 ** -k for k in range(54)]
    # two neighbours on each side of every point where the reduced high word crosses 0x3fe6a09e: sqrt(2)/2 x 2^k
    cross = []
    for k in range(0, -54, -1):
        t = (SQRT_HALF_HI + (k << 20)) << 32
        cross += [t - 2, t - 1, t, t + 1]
    # f = x_reduced - 1 equal to +0, -2^-53, -2^-52 (x_reduced just below 1) and +2^-52, +2^-51 (just above: +2^-53 is
    # not a value of f, the spacing of [1, 2) is 2^-52), at several scales 2^k of x
    small_f = []
    for k in (0, -1, -2, -10, -52, -53):
        s = 2.0 ** k
        small_f += [s, s * (1.0 - 2.0 ** -53), s * (1.0 - 2.0 ** -52)]
        if k < 0:
            small_f += [s * (1.0 + 2.0 ** -52), s * (1.0 + 2.0 ** -51)]
    x = np.concatenate([named, powers, _f64(cross), small_f])
    assert np.all((x > 0.0) & (x <= 1.0)) and np.all(x >= 2.0 ** -1022)
    return x


def test_log_unit_has_the_host_headers_and_the_oracles_bits_on_the_edges_of_its_division():
    from asyncflow_amd.engine import probe_math
    from tests.hostcheck import build as hc

    x = _log_unit_inputs()
    got = probe_math(7, x).view(np.uint64)
    host = hc.math(7, x).view(np.uint64)
    L = ol.lib()
    oracle = np.array([L.orc_x_log(float(v)) for v in x]).view(np.uint64)
    bad = np.flatnonzero(got != host)
    assert bad.size == 0, [(x[i].hex(), hex(got[i]), hex(host[i])) for i in bad[:8]]
    assert np.array_equal(got, oracle)
    assert got[0] == 0                                   # log(1) = +0, not -0


def test_log_unit_has_the_host_headers_bits_on_a_million_draw_arguments():
    from asyncflow_amd.engine import probe_math
    from tests.hostcheck import build as hc

    rng = np.random.default_rng(0x7D7A)
    K = rng.integers(0, 1 << 53, size=1 << 20, dtype=np.uint64)
    x = 1.0 - K.astype(np.float64) * 2.0 ** -53         # (K < 2^53: exact)
    x = x[x > 0.0]
    got = probe_math(7, x).view(np.uint64)
    host = hc.math(7, x).view(np.uint64)
    bad = np.flatnonzero(got != host)
    assert bad.size == 0, [(x[i].hex(), hex(got[i]), hex(host[i])) for i in bad[:8]]
    L = ol.lib()
    some = slice(0, 4096)
    assert np.array_equal(got[some], np.array([L.orc_x_log(float(v)) for v in x[some]]).view(np.uint64))


def test_philox_words_equal_the_oracles_block_for_65536_triples():
    from asyncflow_amd.engine import probe_math

    rng = np.random.default_rng(0xB10C)
    n = 1 << 16
    seeds = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    streams = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    index = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    edge_seeds = [0, 0xFFFFFFFF, 0xFFFFFFFF00000000, 0xFFFFFFFFFFFFFFFF, 0x5EED0007, 0xFFFFFFFF00000001, 0x00000001FFFFFFFF]
    edge_index = [0, 0xFFFFFFFF, 1, 0x80000000]
    edge_streams = [0, 1, 6, 0x1000, 0xFFFFFFFF]
    k = 0
    for s in edge_seeds:
        for i in edge_index:
            for st in edge_streams:
                seeds[k], index[k], streams[k] = s, i, st
                k += 1
    xy = probe_math(8, _f64(seeds), _f64((streams << np.uint64(32)) | index)).view(np.uint64)
    zw = probe_math(9, _f64(seeds), _f64((streams << np.uint64(32)) | index)).view(np.uint64)
    got = np.stack([xy >> np.uint64(32), xy & np.uint64(0xFFFFFFFF), zw >> np.uint64(32), zw & np.uint64(0xFFFFFFFF)], axis=1)
    L = ol.lib()
    out = (C.c_uint32 * 4)()
    want = np.empty((n, 4), dtype=np.uint64)
    for j in range(n):
        sd = int(seeds[j])
        L.orc_x_philox(int(index[j]), 0, int(streams[j]), 0, sd & 0xFFFFFFFF, sd >> 32, out)
        want[j] = out[:]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(hex(int(seeds[j])), int(streams[j]), int(index[j]), got[j], want[j]) for j in bad[:4]]


def test_one_minus_the_uniform_is_the_two_roundings_of_the_plain_text():
    from asyncflow_amd.engine import probe_math

    corners = np.array([0, 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64)
    rng = np.random.default_rng(0x53)
    hi = np.concatenate([np.repeat(corners, 4), rng.integers(0, 1 << 32, size=1 << 16, dtype=np.uint64)])
    lo = np.concatenate([np.tile(corners, 4), rng.integers(0, 1 << 32, size=1 << 16, dtype=np.uint64)])
    # some pairs whose 53 bits are tiny or all ones: 1 - u next to 1 and at 2^-53
    hi = np.concatenate([hi, np.array([0, 0, 0, (1 << 32) - 1], dtype=np.uint64)])
    lo = np.concatenate([lo, np.array([64, 128, 640, (1 << 32) - 64], dtype=np.uint64)])
    got = probe_math(10, _f64((hi << np.uint64(32)) | lo)).view(np.uint64)
    # af::u53 as written: ((double)(hi >> 5) * 2^26 + (double)(lo >> 6)) * 2^-53, then 1.0 - u, each operation rounded
    u = ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)
    want = (1.0 - u).view(np.uint64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(hi[i])), hex(int(lo[i])), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # ... and in integers: 1 - K 2^-53 rounded to nearest even (the independent statement of the same number)
    Kint = ((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))
    exact = np.array([float((1 << 53) - int(kk)) for kk in Kint[:64]]) * 2.0 ** -53   # (2^53 - K <= 2^53: exact in f64)
    assert np.array_equal(got[:64], exact.view(np.uint64))
