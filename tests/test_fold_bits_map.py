"""The field maps of the bit-packed fold image (pmk::FOLD_ROT512Q), restated in numpy.

A coordinate word is an f32 holding 0..255: sign 0, exponent 0 or 127..134, so
exponent bits 6..3 are all equal, and the low half-word is zero.  Its 12-bit
field keeps half-word bits 14 (exponent bit 7), 10 (exponent bit 3) and 9..0;
expanding it copies bit 10 into bits 11..13.  An id word below 2^20 keeps its
low 20 bits.  Both maps select bits, so they are linear over GF(2) and commute
with the XOR of rows: what the fold accumulates in packed form expands to the
parity of the whole rows.  The slice layout (whole quads of four fields per
32-B slice) is restated too, with SIFT1M's 9 slices.
"""
import numpy as np
import pytest


def pack12(x):
    h = x >> np.uint32(16)
    return (h & np.uint32(0x7ff)) | ((h >> np.uint32(3)) & np.uint32(0x800))


def expand12(f):
    h = (f & np.uint32(0x7ff)) | ((f & np.uint32(0x400)) * np.uint32(14)) | ((f & np.uint32(0x800)) << np.uint32(3))
    return h << np.uint32(16)


def pack20(x):
    return x & np.uint32(0xfffff)


def expand20(f):
    return f


def qualifies(x):
    """k_row_bits_or's coordinate test: sign clear, exponent bits 6..3 all equal, low half zero."""
    e = [(x >> np.uint32(23 + b)) & np.uint32(1) for b in range(8)]
    return ((x >> np.uint32(31)) == 0) & (e[6] == e[5]) & (e[6] == e[4]) & (e[6] == e[3]) & ((x & np.uint32(0xffff)) == 0)


BYTES = np.arange(256, dtype=np.float32).view(np.uint32)


def test_every_byte_value_qualifies_and_round_trips():
    assert qualifies(BYTES).all()
    assert np.array_equal(expand12(pack12(BYTES)), BYTES)
    assert pack12(BYTES).max() < 1 << 12
    # 0.0 (exponent 0) and 1.0 (exponent 127: the only value whose bits 6..3 are all ones)
    assert BYTES[0] == 0 and BYTES[1] == 0x3f800000
    e = (BYTES >> np.uint32(23)) & np.uint32(0xff)
    assert [int(v) for v in np.flatnonzero((e >> np.uint32(3)) & np.uint32(0xf) == 0xf)] == [1]


def test_values_that_must_not_qualify():
    # exponents 143 and 119: bits 6..3 are 0001 and 1110; a set sign; a non-zero low half
    for v in (65536.0, 2.0 ** -8, -1.0, 1.0 / 3.0):
        assert not qualifies(np.array([v], dtype=np.float32).view(np.uint32))[0], v
    # 0.5 (exponent 126 = 0b01111110, bits 6..3 all ones like 1.0's) and 256.0 (135 = 0b10000111, all
    # zero like 128.0's) are no bytes but pass the bit test, and their fields expand exactly
    for v in (0.5, 256.0):
        x = np.array([v], dtype=np.float32).view(np.uint32)
        assert qualifies(x)[0] and np.array_equal(expand12(pack12(x)), x), v


def test_ids_round_trip():
    ids = np.random.default_rng(1).integers(0, 1 << 20, size=4096, dtype=np.uint32)
    ids[:2] = (0, (1 << 20) - 1)
    assert np.array_equal(expand20(pack20(ids)), ids)


@pytest.mark.parametrize("nrows", [1, 2, 3, 7, 64, 123, 124])
def test_expand_of_xor_is_xor_of_rows(nrows):
    rng = np.random.default_rng(nrows)
    for trial in range(8):
        v = rng.integers(0, 256, size=(nrows, 128)).astype(np.float32)
        v[0, 0], v[0, 1] = 0.0, 1.0
        if nrows > 1:
            v[1, 0], v[1, 1] = 1.0, 0.0
        c = v.view(np.uint32)
        ids = rng.integers(0, 1 << 20, size=(nrows, 32), dtype=np.uint32)
        assert np.array_equal(expand12(np.bitwise_xor.reduce(pack12(c), axis=0)), np.bitwise_xor.reduce(c, axis=0))
        assert np.array_equal(expand20(np.bitwise_xor.reduce(pack20(ids), axis=0)), np.bitwise_xor.reduce(ids, axis=0))


def slices(w1, n1, w2, n2):
    """Per slice (first coordinate quad, coordinate quads, first other quad, other quads): whole
    quads, 64 // w per slice, the left-over coordinate quads sharing one slice with the first others."""
    per1, per2 = 64 // w1, 64 // w2
    out = [(s * per1, per1, 0, 0) for s in range(n1 // per1)]
    r1, q2 = n1 % per1, 0
    if r1:
        q2 = min((64 - r1 * w1) // w2, n2)
        out.append((n1 - r1, r1, 0, q2))
    while q2 < n2:
        out.append((n1, 0, q2, min(per2, n2 - q2)))
        q2 += per2
    return out


@pytest.mark.parametrize("w1,w2,dim,m,want", [
    (12, 20, 128, 32, 9), (16, 20, 128, 32, 11), (12, 32, 128, 32, 11),   # SIFT1M: 12 as FOLD_ROT512P
    (12, 20, 64, 32, 6), (16, 20, 64, 32, 7), (12, 20, 64, 8, 4), (12, 20, 32, 8, 3),
])
def test_slice_layout(w1, w2, dim, m, want):
    sl = slices(w1, dim // 4, w2, m // 4)
    assert len(sl) == want
    assert all(c1 * 4 * w1 + c2 * 4 * w2 <= 256 for _, c1, _, c2 in sl)
    assert sum(c1 for _, c1, _, _ in sl) == dim // 4 and sum(c2 for *_, c2 in sl) == m // 4
    # every quad in exactly one slice, in order
    assert [q for q1, c1, _, _ in sl for q in range(q1, q1 + c1)] == list(range(dim // 4))
    assert [q for _, _, q2, c2 in sl for q in range(q2, q2 + c2)] == list(range(m // 4))
