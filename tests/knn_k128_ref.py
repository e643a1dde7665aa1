"""The data of the 128-key exact kNN's tests (pm_graph.hip, DESIGN.md
§10.3).  numpy only: no GPU, none of the code under test.  The value families,
the padding rule and the bound are tests/knn_ref.py's and tests/knn_wide_ref.py's;
tests/test_abi_k128.py checks, with this module and the oracle alone, the
conditions the generators promise."""
import numpy as np

from tests.knn_wide_ref import (EMPTY, F32, K_MID, c_dp, clustered_floats, descending_rows, dist64,  # noqa: F401
                                eps_bound, huge_row_data, norms64, oracle_dist, pad_dim, pref_family, shape_data)

TOP = 128   # prefilter keys per query row

SHAPE_N = (1, 64, 65, 127, 128, 129, 193, 257)
SHAPE_NQ = (1, 63, 64, 65, 130)
SHAPE_DIM = (1, 7, 8, 128, 129, 192, 193, 256, 320, 960, 1023, 1024)   # six narrow, six wide
SHAPE_K = (1, 64, 65, 100, 127, 128, "n+1")


def shape_cases():
    """32 (n, nq, dim, k, integer) cases: n walks its eight values four times,
    dim its twelve at least twice and nq its five at least six times (shifted
    every round, so that the pairs change); k walks 1, 64, 65, 100, 127, 128 and
    n + 1 (K_MID where n + 1 > 128); floats and integers 0..255 alternate
    while dim shifts by one every round, so that every dim sees both."""
    out = []
    for i in range(32):
        n = SHAPE_N[i % 8]
        nq = SHAPE_NQ[(i + i // 8) % 5]
        dim = SHAPE_DIM[(i + i // 12) % 12]
        k = SHAPE_K[(i + i // 7) % 7]
        if k == "n+1":
            k = n + 1 if n + 1 <= TOP else K_MID
        out.append((n, nq, dim, k, bool(i % 2)))
    return out


def identical_rows(dim, n=450, copies=300, seed=3):
    """(v, q, ntie): `copies` identical rows in two runs (ids 10 .. 159 and the
    last 150), more than 128 ties at every key of their queries; q[0:3] equal to
    them, q[3:] equal to other base rows; ntie = 3."""
    rng = np.random.default_rng([seed, dim])
    v = rng.standard_normal((n, dim)).astype(F32)
    row = rng.standard_normal(dim).astype(F32)
    v[10:10 + copies // 2] = row
    v[n - copies // 2:] = row
    q = np.stack([row, row, row, v[0], v[5], v[200], v[250]])
    return v, q, 3


NEAR_DUP = 100   # between 64 and 128


def near_tie_rows(dim, n=300, seed=5):
    """(v, q, ntie): the first 100 rows lie within a few ulps of one row, the last
    row is twice as long as a typical one (it sets the certificate's eps); q[0:4]
    are among the 100, q[4:] elsewhere; ntie = 4.  For q[0:4] the 48th and the
    64th distance are both about 0 while the 128th is about 2 dim: 64 keys cannot
    certify k = 48, 128 keys can (subset_verdict)."""
    rng = np.random.default_rng([seed, dim])
    base = rng.standard_normal(dim).astype(F32)
    v = rng.standard_normal((n, dim)).astype(F32)
    for i in range(NEAR_DUP):
        r = base.copy()
        r[i % dim] = r[i % dim] + F32(1 + i // dim) * np.spacing(r[i % dim])
        v[i] = r
    v[n - 1] = v[n - 1] * F32(2)
    q = np.concatenate([v[[0, 3, 40, 99]], v[[120, 150, 200, 250, 298]] + F32(0.5)]).astype(F32)
    return v, q, 4


def subset_verdict(oracle, v, q, k):
    """(sure64, sure128) per query row, from float64 distances and the oracle's
    L2Dist alone.  E = c_dp (|q|^2 + max |x|^2) + 2^-50 bounds every prefilter
    error and is at most the kernel's eps (which is at most 1.001 E).
    sure64: the 64 nearest rows have prefilter distances <= D_64 + e64, e64 the
    bound with the largest norm among those 64, so tau_64 - eps <= D_64 + e64 - E;
    the row is uncertified with 64 keys if d_k is not below that.
    sure128: tau_128 >= D_128 - E, so the row is certified with 128 keys if d_k <
    D_128 - 2.001 E."""
    dp = pad_dim(v.shape[1])
    qn, xn = norms64(q), norms64(v)
    D = dist64(q, v)
    order = np.argsort(D, axis=1, kind="stable")
    Ds = np.take_along_axis(D, order, axis=1)
    E = eps_bound(dp, qn, xn.max())
    e64 = eps_bound(dp, qn, xn[order[:, :64]].max(axis=1))
    dk = oracle.knn(v, q, k)[1][:, k - 1].astype(np.float64)
    sure64 = dk >= Ds[:, 63] + e64 - E
    sure128 = dk < Ds[:, TOP - 1] - 2.001 * E
    return sure64, sure128
