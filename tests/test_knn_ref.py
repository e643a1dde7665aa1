"""The conditions the generators of tests/knn_ref.py promise to the GPU tests
(tests/test_gpu_knn_stages.py, test_gpu_knn_exact.py, test_gpu_prune.py),
checked with that module and the oracle alone."""
import itertools

import numpy as np
import pytest

from tests import knn_ref as R


def test_bf16_rounding_known_values():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 3.0e38], dtype=np.float32)
    #             exact  halfway->even(down)  halfway->even(up)
    assert R.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBF80, 0x0000, 0x8000, 0x7F62]
    assert R.bf16_to_f32(np.array([0x3F80, 0xC000], np.uint16)).tolist() == [1.0, -2.0]


def test_fixed_order_norm_is_not_the_plain_sum():
    """The butterfly order is a definite order: exact on integers, and on
    full-mantissa rows it differs from numpy's own sum somewhere."""
    v = np.arange(192, dtype=np.float32)[None, :] % 7
    assert R.norms_fixed_order(v)[0] == float((v.astype(np.float64) ** 2).sum())
    x = R.split_family("mantissa24", 40, 192)
    a = R.norms_fixed_order(x)
    assert a.dtype == np.float32
    assert np.allclose(a, R.norms64(x), rtol=2e-6)
    seq = np.zeros(40, np.float32)
    for c in range(192):
        seq = seq + x[:, c] * x[:, c]
    assert (a != seq).any()


def test_c_dp_values():
    assert abs(R.c_dp(128) - 1.17e-4) < 1e-6 and abs(R.c_dp(192) - 1.62e-4) < 1e-6
    assert R.c_dp(192) < 2.0 ** -12


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 128, 129, 192])
def test_split_families(dim):
    n = 50
    fam = {f: R.split_family(f, n, dim) for f in R.SPLIT_FAMILIES}
    for f, x in fam.items():
        assert x.shape == (n, dim) and x.dtype == np.float32 and np.isfinite(x).all(), f
    bits = {f: x.view(np.uint32) for f, x in fam.items()}
    assert (bits["mantissa24"] & 1).all()
    for f, odd in (("halfway_even", 0), ("halfway_odd", 1)):
        assert ((bits[f] & 0xFFFF) == 0x8000).all()
        assert (((bits[f] >> 16) & 1) == odd).all()
        # the tie goes to the even neighbour: down for even, up for odd
        assert (R.bf16_bits(fam[f]) == ((bits[f] >> 16) + odd).astype(np.uint16)).all()
    z = bits["zeros"]
    assert ((z & 0x7FFFFFFF) == 0).all()
    if dim > 1:
        assert (z == 0).any() and (z == 0x80000000).any()
    s = bits["subnormal"]
    assert ((s >> 23) & 0xFF == 0).all() and ((s & 0x7FFFFF) != 0).all()
    hi, lo = R.split_rows(fam["lo_subnormal"])
    lo = lo[:, :dim]
    assert (((bits["lo_subnormal"] >> 23) & 0xFF) != 0).all()          # x itself is normal
    assert (((lo >> 7) & 0xFF) == 0).all() and ((lo & 0x7F) != 0).any()   # its lo is a bf16 subnormal
    mixed = R.split_rows_mixed(dim)
    assert mixed.shape == (6 * len(R.SPLIT_FAMILIES), dim)
    hi, lo = R.split_rows(mixed)
    assert hi.shape == (len(mixed), R.pad_dim(dim)) and not hi[:, dim:].any() and not lo[:, dim:].any()
    # hi + lo reproduces x to 2^-16 relative (2^-133 absolute: bf16's subnormal step)
    back = R.bf16_to_f32(hi[:, :dim]).astype(np.float64) + R.bf16_to_f32(lo[:, :dim]).astype(np.float64)
    assert (np.abs(back - mixed) <= 2.0 ** -16 * np.abs(mixed) + 2.0 ** -133).all()


@pytest.mark.parametrize("dim", R.PREF_DIMS)
def test_prefilter_families(oracle, dim):
    dp = R.pad_dim(dim)
    for f in R.PREF_FAMILIES:
        q, x = R.pref_family(f, dim)
        assert q.shape == (R.PREF_NQ, dim) and x.shape == (R.PREF_N, dim) and R.PREF_N <= 64, f
        assert q.dtype == x.dtype == np.float32 and np.isfinite(q).all() and np.isfinite(x).all()
        qn, xn = R.norms64(q), R.norms64(x)
        S = qn[:, None] + xn[None, :]
        assert S.max() < R.MAX_SUM, f
        if f == "positive":
            assert (q >= 1).all() and (x >= 1).all() and (q.view(np.uint32) & 1).all() and (x.view(np.uint32) & 1).all()
        if f == "alternating":
            p = np.sign(q[0] * x[0])
            assert (p[::2] == 1).all() and (p[1::2] == -1).all()
        if f == "near":
            d = R.dist64(q, x)
            pair = d[np.arange(R.PREF_N), np.arange(R.PREF_N)]
            assert (pair < 2.0 ** -30 * S[np.arange(R.PREF_N), np.arange(R.PREF_N)]).all()
            assert (pair > 0).any()
        if f == "integer":
            assert ((q == np.floor(q)) & (q >= 0) & (q <= 255)).all() and ((x == np.floor(x)) & (x >= 0) & (x <= 255)).all()
            assert np.array_equal(R.oracle_dist(oracle, q, x).astype(np.float64), R.dist64(q, x))
        if f == "scale_2^-70":    # the absolute term is the bound
            assert (R.c_dp(dp) * S).max() < 2.0 ** -20 * R.ABS_TERM
        if f == "scale_2^58":
            assert S.max() < R.MAX_SUM and S.max() > 2.0 ** 110
        if f in R.PREF_SCALES:
            q0, x0 = R.pref_family("normal", dim)
            assert q0.shape == q.shape and (np.abs(q[q != 0]) < np.inf).all()
            assert np.array_equal(np.frexp(q)[0], np.frexp(R.pref_family(f, dim)[0])[0])


def test_premise_data():
    for d in (100, 192):
        v, q = R.clustered_floats(1000, d, nq=50)
        assert v.shape == (1000, d) and q.shape == (13, d)
    v, q = R.near_duplicate_rows()
    assert v.shape == (300, 100) and q.shape == (9, 100)
    # more than 64 rows within a few ulps of the first four queries
    assert (R.dist64(q[:4], v[:100]) < 1e-8).all()


def test_shape_cases_cover():
    cases = R.shape_cases()
    assert len(cases) == 40 and len(set(cases)) == 40
    cols = list(zip(*cases))
    assert set(cols[0]) == set(R.SHAPE_N) and set(cols[1]) == set(R.SHAPE_NQ) and set(cols[2]) == set(R.SHAPE_DIM)
    assert set(cols[4]) == {0, 1, 2}
    for n, nq, dim, k, kc in cases:
        assert 1 <= k <= 64
        assert k == (1, 64)[kc] if kc < 2 else (k == n + 1 if n < 63 else k == R.K_MID)
    assert {(1, 2), (1, 64), (63, 64)} <= {(c[0], c[3]) for c in cases}   # k > n: -1 / +inf padding
    pairs = lambda a, b: {(c[a], c[b]) for c in cases}   # noqa: E731
    assert len(pairs(0, 1)) == 40 and len(pairs(0, 4)) == 24 and len(pairs(1, 4)) == 15 and len(pairs(2, 4)) == 27
    assert len(pairs(0, 2)) == 40 and len(pairs(1, 2)) == 40
    for integer in (False, True):
        v, q = R.shape_data(65, 63, 9, integer)
        assert v.shape == (65, 9) and q.shape == (63, 9) and np.array_equal(v[5], v[3]) and np.array_equal(q[:8], v[:8])
        if integer:
            assert ((v == np.floor(v)) & (v >= 0) & (v <= 255)).all()


@pytest.mark.parametrize("integer", [False, True])
def test_descending_rows(oracle, integer):
    v, q = R.descending_rows(integer)
    assert v.shape == (R.DESC_N, 128) and R.DESC_N == 1024
    d = oracle.l2_batch(q[0], v)
    assert (np.diff(d.astype(np.float64)) < 0).all()      # strictly decreasing in id
    if integer:
        assert ((v == np.floor(v)) & (v >= 0) & (v <= 255)).all()
        assert d.tolist() == list(range(1024, 0, -1))
    d = oracle.l2_batch(q[0], np.ascontiguousarray(v[::-1]))   # the mirror ascends
    assert (np.diff(d.astype(np.float64)) > 0).all()


@pytest.mark.parametrize("integer", [False, True])
def test_tie_rows(oracle, integer):
    v, q, nt = R.identical_rows(integer)
    d = R.oracle_dist(oracle, q, v)
    assert nt == 3 and ((d[:nt] == 0).sum(axis=1) == 200).all()
    assert ((d[nt:] == 0).sum(axis=1) == 1).all()          # the other queries equal one base row each
    assert (np.sort(d[nt:], axis=1)[:, 1] > 1).all()       # which stands alone
    v, q, nt = R.equidistant_rows(integer)
    d = R.oracle_dist(oracle, q, v).view(np.uint32)
    lowest = d.min(axis=1)
    assert (lowest != 0).all()
    tied = d == lowest[:, None]
    assert nt == 2 and (tied.sum(axis=1) == 200).all() and tied.sum(axis=1).min() >= 65
    assert tied[0, :100].all() and tied[0, -100:].all()    # early and late tiles
    if integer:
        assert ((v == np.floor(v)) & (v >= 0) & (v <= 255)).all()


def test_prune_generators(oracle):
    X = R.collinear_points(40)
    for m, alpha in itertools.product((8, 32), (1.0, 1.2, 2.0)):
        cand = np.arange(1, 41, dtype=np.uint32)
        acc, disc, _ = R.prune_trace(oracle, X, 0, cand, m, alpha)
        assert acc == [1] and disc == list(range(2, 41))          # exactly one accept
        assert oracle.robust_prune(X, 0, cand, m, alpha).tolist() == [1] + list(range(2, m + 1))
    X, cand, w, j = R.late_rejector()
    for alpha in (1.0, 1.2, 2.0):
        acc, disc, _ = R.prune_trace(oracle, X, 0, cand, 42, alpha)
        assert acc == list(range(1, 43)) and disc == [w] and j >= 32
        assert oracle.robust_prune(X, 0, cand, 42, alpha).tolist() == acc
        d = oracle.l2_batch(X[w], X[np.array(acc[:40], dtype=np.uint32)]) * np.float32(alpha)
        assert np.flatnonzero(d < oracle.l2_batch(X[0], X[w:w + 1])[0]).tolist() == [j]   # its only rejector
    X, cand = R.hub_discards()
    acc, disc, before =R.prune_trace(oracle, X, 0, cand, 8, 1.2)
    assert len(acc) == 8 and before > 4096 and before == len(disc) == 4099
    assert oracle.robust_prune(X, 0, cand, 8, 1.2).tolist() == acc == [1] + list(range(4101, 4108))
    # the trace is the oracle's own pass on ordinary data too
    rng = np.random.default_rng(1)
    X = rng.standard_normal((300, 8)).astype(np.float32)
    for u in range(5):
        cand = rng.integers(0, 300, 90).astype(np.uint32)
        acc, disc, _ = R.prune_trace(oracle, X, u, cand, 32, 1.2)
        assert (acc + disc[:32 - len(acc)] if len(acc) < 32 else acc) == oracle.robust_prune(X, u, cand, 32, 1.2).tolist()
