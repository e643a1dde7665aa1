"""The arithmetic and the data of the uint8 exact kNN's tests (pm_graph_u8.hip,
DESIGN.md §10.4).  numpy only: no GPU, none of the code under test.

biased_distances restates the identity the kernels rest on: rows stored as
x' = x - 128 (int8), padded with 0 to a multiple of 64, acc = sum x' q' from the
matrix core, and

    q.x  = acc + 128 (sum q + sum x) - 128^2 dim
    dist = |q|^2 + |x|^2 - 2 q.x = c(q) + c(x) - 2 acc,
    c(v) = |v|^2 - 256 sum v + 128^2 dim        (= sum (v - 128)^2)

in int64, and reports the largest magnitude of every intermediate so that a test
can check that all of them fit int32 and that dist < 2^24 (exact in float32)."""
import numpy as np

from tests.knn_ref import descending_rows as _descending_rows

TOP = 128        # keys per query row
MAX_DIM = 256    # 256 * 255^2 = 16,646,400 < 2^24
MAX_DIST = 256 * 255 * 255

SHAPE_N = (1, 63, 64, 65, 127, 128, 129, 193, 1000)
SHAPE_NQ = (1, 63, 64, 65, 130)
SHAPE_DIM = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256)
SHAPE_K = (1, 64, 128, "n+1")


def pad_dim(dim):
    return -(-dim // 64) * 64


def biased_distances(q, x):
    """(dist [nq][n] int64, peak): the squared distances of uint8 rows q and x by
    the biased identity; peak maps each intermediate's name to its largest
    magnitude."""
    assert q.dtype == np.uint8 and x.dtype == np.uint8 and q.shape[1] == x.shape[1]
    dim = q.shape[1]
    dp = pad_dim(dim)

    def operand(v):
        b = np.zeros((len(v), dp), np.int64)
        b[:, :dim] = (v ^ 0x80).view(np.int8)      # x ^ 0x80 read as int8 is x - 128
        assert np.array_equal(b[:, :dim], v.astype(np.int64) - 128)
        return b

    qb, xb = operand(q), operand(x)
    acc = qb @ xb.T
    q64, x64 = q.astype(np.int64), x.astype(np.int64)
    sq, sx = q64.sum(1), x64.sum(1)
    nq, nx = (q64 * q64).sum(1), (x64 * x64).sum(1)
    qx = acc + 128 * (sq[:, None] + sx[None, :]) - 128 * 128 * dim
    assert np.array_equal(qx, q64 @ x64.T)
    dist = nq[:, None] + nx[None, :] - 2 * qx
    cq = nq - 256 * sq + 128 * 128 * dim
    cx = nx - 256 * sx + 128 * 128 * dim
    assert np.array_equal(cq, (qb * qb).sum(1)) and np.array_equal(cx, (xb * xb).sum(1))
    folded = cq[:, None] + cx[None, :] - 2 * acc
    assert np.array_equal(folded, dist)
    peak = {name: int(np.abs(a).max()) for name, a in
            (("acc", acc), ("2acc", 2 * acc), ("sum", sq[:, None] + sx[None, :]), ("128sum", 128 * (sq[:, None] + sx[None, :])),
             ("norms", nq[:, None] + nx[None, :]), ("qx", qx), ("2qx", 2 * qx), ("cq", cq), ("cx", cx),
             ("cq+cx", cq[:, None] + cx[None, :]), ("dist", dist))}
    return dist, peak


def rank(dist, k):
    """(ids [nq][k] int64, dists [nq][k] float32) of the (dist, id) ranking, -1 and
    +inf beyond n."""
    nq, n = dist.shape
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    ids = np.full((nq, k), -1, np.int64)
    d = np.full((nq, k), np.inf, np.float32)
    ids[:, :order.shape[1]] = order
    d[:, :order.shape[1]] = np.take_along_axis(dist, order, axis=1).astype(np.float32)
    return ids, d


def shape_cases():
    """45 (n, nq, dim, k) cases: n walks its nine values five times, nq its five
    (shifted every round of nine, so that the pairs change), dim its twelve
    (shifted every round of twelve); k walks 1, 64, 128 and min(n + 1, 128)."""
    out = []
    for i in range(45):
        n = SHAPE_N[i % 9]
        nq = SHAPE_NQ[(i + 2 * (i // 9)) % 5]
        dim = SHAPE_DIM[(i + i // 12) % 12]
        k = SHAPE_K[(i + i // 4) % 4]
        out.append((n, nq, dim, min(n + 1, TOP) if k == "n+1" else k))
    return out


def shape_data(n, nq, dim, seed=0):
    """Random bytes; row 5 repeats row 3 (a tie by id) where they exist; the first
    queries are base rows."""
    rng = np.random.default_rng([seed, n, nq, dim])
    v = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    if n > 5:
        v[5] = v[3]
    q = rng.integers(0, 256, (nq, dim), dtype=np.uint8)
    m = min(n, nq, 8)
    q[:m] = v[:m]
    return v, q


def extreme_rows():
    """(v [72][256], q [4][256]): rows of all 0, all 255, 0/255 and 255/0
    alternating, each 16 times between 8 random rows, and the four as queries:
    the largest acc of both signs (+-256 * 128^2), the largest constants and the
    largest distance (256 * 255^2)."""
    lo, hi = np.zeros(256, np.uint8), np.full(256, 255, np.uint8)
    alt = np.where(np.arange(256) % 2 == 0, 0, 255).astype(np.uint8)
    pats = np.stack([lo, hi, alt, 255 - alt])
    rnd = np.random.default_rng(17).integers(0, 256, (8, 256), dtype=np.uint8)
    v = np.concatenate([np.tile(pats, (8, 1)), rnd, np.tile(pats, (8, 1))])
    return np.ascontiguousarray(v), pats


def descending_rows():
    """(v [1024][128], q [1][128]) bytes: the distance to q = 0 strictly decreases
    with the id (knn_ref.descending_rows' integers)."""
    v, q = _descending_rows(True)
    return v.astype(np.uint8), q.astype(np.uint8)


def identical_rows(dim=100, n=450, copies=300, seed=3):
    """(v, q, ntie): `copies` identical rows in two runs (ids 10 .. 159 and the
    last 150): more than 128 ties at distance 0; q[0:3] equal to them, q[3:] to
    other base rows; ntie = 3."""
    rng = np.random.default_rng([seed, dim])
    v = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    row = rng.integers(0, 256, dim, dtype=np.uint8)
    v[10:10 + copies // 2] = row
    v[n - copies // 2:] = row
    q = np.stack([row, row, row, v[0], v[5], v[200], v[250]])
    return v, q, 3


def one_distance_rows(n=1000, dim=256, seed=4):
    """(v, q): 200 rows at distance 1 from q[0] (one coordinate each, one step
    up), ids 0 .. 99 (the first tiles) and n - 100 .. n - 1 (the last); the
    other rows random, far away.  q[1] is a random row."""
    rng = np.random.default_rng([seed, dim])
    v = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    row = rng.integers(0, 255, dim, dtype=np.uint8)
    ids = np.concatenate([np.arange(100), np.arange(n - 100, n)])
    for j, i in enumerate(ids):
        v[i] = row
        v[i, j] += 1
    return v, np.stack([row, v[500]]), ids
