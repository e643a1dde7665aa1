"""The plain reference of the wide exact kNN's stages (pm_graph.hip,
DESIGN.md §10.2) and the data of its edge tests.  numpy only: no GPU, none of
the code under test.  The value families, the bound and the robustPrune data
are tests/knn_ref.py's; the padding rule and the split / norm order are
restated here for the wide dp, because knn_ref.pad_dim knows only 128 and 192."""
import numpy as np

from tests.knn_ref import (ABS_TERM, EMPTY, F32, K_MID, MAX_SUM, PREF_FAMILIES, PREF_N, PREF_NQ,  # noqa: F401
                           SPLIT_FAMILIES, bf16_bits, bf16_to_f32, c_dp, clustered_floats, collinear_points, dist64,
                           eps_bound, hub_discards, late_rejector, norms64, oracle_dist, pref_family, prune_trace,
                           split_rows_mixed)

MAX_DIM = 1024
CHUNK = 64   # the prefilter's K chunk and the norm's wave width


def pad_dim(dim):
    """128 and 192 as the narrow path; above 192 the next multiple of 64."""
    assert 1 <= dim <= MAX_DIM
    if dim <= 128:
        return 128
    if dim <= 192:
        return 192
    return -(-dim // CHUNK) * CHUNK


def split_rows(rows):
    """hi = bf16(x), lo = bf16(f32(x - hi)) as uint16 [n][dp], zero padded."""
    x = np.ascontiguousarray(rows, dtype=F32)
    n, dim = x.shape
    dp = pad_dim(dim)
    hi = np.zeros((n, dp), np.uint16)
    lo = np.zeros((n, dp), np.uint16)
    hi[:, :dim] = bf16_bits(x)
    lo[:, :dim] = bf16_bits(x - bf16_to_f32(hi[:, :dim]))
    return hi, lo


def norms_fixed_order(rows):
    """The kernel's norm: per 64-wide chunk an xor-butterfly tree over the f32
    squares (lane l adds lane l ^ o for o = 1, 2, .. 32), then the dp / 64 chunks
    added in order to a sum that starts at 0; float32 throughout."""
    x = np.ascontiguousarray(rows, dtype=F32)
    n, dim = x.shape
    dp = pad_dim(dim)
    p = np.zeros((n, dp), F32)
    p[:, :dim] = x
    sq = (p * p).reshape(n, dp // 64, 64)
    lane = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        sq = sq + sq[:, :, lane ^ o]
    s = np.zeros(n, F32)
    for c in range(dp // 64):
        s = s + sq[:, c, 0]
    assert s.dtype == F32
    return s


# --------------------------------------------------------------------------
# end-to-end shapes
# --------------------------------------------------------------------------
SHAPE_DIM = (193, 255, 256, 257, 320, 511, 512, 960, 1023, 1024)
SHAPE_NNQ = ((1, 1), (63, 65), (64, 64), (65, 1), (129, 130), (193, 63))


def shape_cases():
    """20 (n, nq, dim, k, integer) cases: dim walks its ten values twice, (n, nq)
    its six pairs at least three times; k walks 1, 64 and n + 1 (where that is
    <= 64, else K_MID); floats and integers 0..255 alternate, shifted in the
    second round so that every dim sees both."""
    out = []
    for i in range(20):
        n, nq = SHAPE_NNQ[i % 6]
        k = (1, 64, n + 1 if n + 1 <= 64 else K_MID)[(i + i // 6) % 3]
        out.append((n, nq, SHAPE_DIM[i % 10], k, bool((i + i // 10) % 2)))
    return out


def shape_data(n, nq, dim, integer, seed=0):
    """Rows for a shape case: N(0,1) floats or integers 0..255; row 5 repeats
    row 3 (a tie by id) where they exist; the first queries are base rows."""
    rng = np.random.default_rng([seed, n, nq, dim, int(integer)])
    gen = (lambda r, c: rng.integers(0, 256, (r, c)).astype(F32)) if integer else \
        (lambda r, c: rng.standard_normal((r, c)).astype(F32))
    v = gen(n, dim)
    if n > 5:
        v[5] = v[3]
    q = gen(nq, dim)
    m = min(n, nq, 8)
    q[:m] = v[:m]
    return v, q


DESC_N = 1024


def descending_rows(dim=256):
    """(v [1024][dim], q [1][dim]) as knn_ref.descending_rows' floats: v_i = (2 -
    i / 1024) u for a fixed direction u, q = -u, so L2Dist(q, v_i) strictly
    decreases with i and every tile of the prefilter inserts all its columns."""
    u = np.random.default_rng(21).standard_normal(dim).astype(F32)
    s = (F32(2) - np.arange(DESC_N, dtype=F32) / F32(DESC_N))
    return (s[:, None] * u[None, :]).astype(F32), -u[None, :]


def identical_rows(n=330, dim=200, copies=200, seed=3):
    """(v, q, ntie): `copies` identical rows in two runs (ids 10.. and the last
    ones), q[0:3] equal to them, q[3:] equal to other base rows; ntie = 3."""
    rng = np.random.default_rng([seed, dim])
    v = rng.standard_normal((n, dim)).astype(F32)
    row = rng.standard_normal(dim).astype(F32)
    v[10:10 + copies // 2] = row
    v[n - copies // 2:] = row
    q = np.stack([row, row, row, v[0], v[5], v[150], v[200]])
    return v, q, 3


def huge_row_data(dim, n=300, nq=9, seed=6):
    """Unit-scale rows with one row of norm about 2^100: eps follows the largest
    norm, so no query row can be certified."""
    rng = np.random.default_rng([seed, dim])
    v = rng.standard_normal((n, dim)).astype(F32)
    q = rng.standard_normal((nq, dim)).astype(F32)
    v[n // 2] = v[n // 2] * F32(2.0 ** 50) / np.sqrt(F32(dim))   # |x|^2 about 2^100
    return v, q
