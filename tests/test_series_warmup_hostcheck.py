"""The exact arithmetic of the warm-up analyzer on the host, under AddressSanitizer + UBSan: tests/hostcheck/warmup_check.cpp is
a stand-alone program over asyncflow_amd/csrc/af_wide.hpp (256-bit add, subtract, both multiplies, compare) and the per-cell
routine of asyncflow_amd/csrc/af_series_warmup.hpp (afwu::cell_of: the 64 lanes of the device's wave one after the other).
It runs as a child process and everything it prints is compared with Python integers.  The cell sequences reach batch sums
near 2^64 over 2^20 batches: compared products of more than 220 bits, which no device test of a few seconds reaches."""

from __future__ import annotations

import os
import random
import struct
import subprocess

import numpy as np
import pytest

from asyncflow_amd.results import warmup_truncation
from tests.hostcheck import build as hc

_problem = hc.sanitizer_link_problem()
pytestmark = pytest.mark.skipif(_problem is not None, reason=str(_problem))

M256 = (1 << 256) - 1
SRC = hc.HERE / "warmup_check.cpp"
HEADERS = [hc.ROOT / "asyncflow_amd/csrc/af_wide.hpp", hc.ROOT / "asyncflow_amd/csrc/af_series_warmup.hpp"]


@pytest.fixture(scope="module")
def program():
    exe = hc.SAN_DIR / "warmup_check"
    hc.SAN_DIR.mkdir(exist_ok=True)
    newest = max(p.stat().st_mtime for p in (SRC, *HEADERS))
    if not exe.exists() or exe.stat().st_mtime < newest:
        subprocess.run(["g++", *hc.SAN_FLAGS, "-Wall", "-o", str(exe), str(SRC)], check=True, capture_output=True, text=True)
    return exe


def _run(program, mode: str, data: bytes) -> list[str]:
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(program), mode], input=data, capture_output=True, env={**env, **hc.SAN_ENV}, timeout=240, check=False)
    err = r.stderr.decode()
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert r.returncode == 0, (r.returncode, err[-4000:])
    return r.stdout.decode().splitlines()


def _limbs(v: int) -> list[int]:
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def _value(words: list[str]) -> int:
    return sum(int(w, 16) << (64 * i) for i, w in enumerate(words))


def test_wide_operations_equal_python_integers(program):
    rnd = random.Random(256)
    top = 0xFFFFFFFFFFFFFFFF
    pairs = [(0, 0), (M256, 1), (1, M256), (M256, M256), (top, 1), ((1 << 128) - 1, 1), ((1 << 192) - 1, 1), (1 << 64, 1), (1 << 128, 1),
             (1 << 192, 1), (1 << 255, 1 << 255), ((1 << 178) - 1, (1 << 75) - 1), ((1 << 89) - 1, (1 << 89) - 1), (top, top | (top << 64))]
    for k in range(4):                                   # a carry / borrow out of limb k that runs through the limbs above it
        pairs += [(((1 << 256) - 1) >> (64 * (3 - k)), 1), (1 << (64 * (k + 1)) if k < 3 else 0, 1), ((top << (64 * k)) & M256, top << (64 * k) & M256)]
    for _ in range(3000):
        bits_a, bits_b = rnd.choice((1, 63, 64, 65, 127, 128, 129, 178, 191, 192, 193, 253, 255, 256)), rnd.choice((1, 32, 64, 75, 89, 128, 200, 256))
        a, b = rnd.getrandbits(bits_a), rnd.getrandbits(bits_b)
        if rnd.random() < 0.2:                           # limbs of all ones: every carry travels
            a |= top << (64 * rnd.randrange(4))
            a &= M256
        pairs.append((a, b))
        pairs.append((b, a))
    text = "".join(" ".join(f"{w:x}" for w in _limbs(a) + _limbs(b)) + "\n" for a, b in pairs)
    lines = _run(program, "ops", text.encode())
    assert len(lines) == len(pairs)
    carried = np.zeros(4, dtype=np.int64)
    for (a, b), line in zip(pairs, lines):
        w = line.split()
        assert len(w) == 17
        b0, b01 = b & top, b & ((1 << 128) - 1)
        assert _value(w[0:4]) == (a + b) & M256, ("add", hex(a), hex(b))
        assert _value(w[4:8]) == (a - b) & M256, ("sub", hex(a), hex(b))
        assert _value(w[8:12]) == (a * b0) & M256, ("mul_u64", hex(a), hex(b0))
        assert _value(w[12:16]) == (a * b01) & M256, ("mul_u128", hex(a), hex(b01))
        assert int(w[16]) == (a > b) - (a < b), ("cmp", hex(a), hex(b))
        for k in range(4):
            low = (1 << (64 * (k + 1))) - 1
            carried[k] += (a & low) + (b & low) > low
    assert (carried > 0).all(), carried                  # an addition carried out of every limb


def _walk(y: list[int]) -> tuple[tuple[int, int, int, int, int], int]:
    """warmup_truncation, and the largest product its comparisons form."""
    J = len(y)
    s1, s2 = sum(y), sum(v * v for v in y)
    best, largest = (0, J * s2 - s1 * s1, J ** 3), 0
    for d in range(1, J // 2 + 1):
        s1 -= y[d - 1]
        s2 -= y[d - 1] ** 2
        m = J - d
        a = m * s2 - s1 * s1
        left, right = a * best[2], best[1] * m ** 3
        largest = max(largest, left, right)
        if left < right:
            best = (d, a, m ** 3)
    return warmup_truncation(y), largest


def test_cells_equal_python_integers_past_192_bit_products(program):
    rnd = np.random.default_rng(2 ** 20)
    top = (1 << 64) - 1
    seqs: list[list[int]] = [[], [7], [top], [3, 3], [1, 2, 3], [5, 9, 1, 7] + [3] * 60, [4] * 64, [4] * 65, [top] * 200,
                             [0] * 100 + [1] * 100, [top, 0] * 64, list(range(1, 130))]
    for J in (2, 63, 64, 65, 127, 128, 129, 1000, 4097):
        seqs.append(rnd.integers(0, 1 << 20, J).tolist())
        seqs.append([int(v) for v in rnd.integers(0, 1 << 63, J).astype(object) * 2 + 1])
    # near 2^64 over 2^20 batches: a transient of half-size values, then values within 2^40 of the top, and a planted tie
    J = 1 << 20
    big = (top - rnd.integers(0, 1 << 40, J).astype(object))
    big[: J // 7] = big[: J // 7] // 3
    seqs.append([int(v) for v in big[: 1 << 18]])
    seqs.append([int(v) for v in (top - rnd.integers(0, 1 << 62, 1 << 17).astype(object))])
    flat = [int(v) for v in big]
    flat[J // 3:] = [top] * (J - J // 3)                 # constant from a batch on: A = 0 from there, the smallest such d wins
    seqs.append(flat)
    data = b"".join(struct.pack("<I", len(y)) + np.array(y, dtype=np.uint64).tobytes() for y in seqs)
    lines = _run(program, "cells", data)
    assert len(lines) == len(seqs)
    most = 0
    for y, line in zip(seqs, lines):
        w = line.split()
        want, largest = _walk(y)
        got = (int(w[0]), _value(w[1:5]), _value(w[5:9]), _value(w[9:13]), _value(w[13:17]))
        assert got == want, (len(y), got[0], want[0])
        most = max(most, largest)
    assert lines[5].split()[0] == "4" and lines[-1].split()[0] == str(J // 3)
    print(f"largest compared product: {most.bit_length()} bits")
    assert most > 1 << 192 and most < 1 << 253
