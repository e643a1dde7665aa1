"""The plain reference of the exact kNN's stages (pm_graph.hip)
and the data of the kNN and robustPrune edge tests.  numpy only: no GPU, none
of the code under test.  tests/test_knn_ref.py checks, with this module and the
oracle alone, the conditions each generator promises."""
import numpy as np

F32 = np.float32
EMPTY = 0xFFFFFFFF   # an empty candidate slot


# --------------------------------------------------------------------------
# the stages of k_to_bf16x2 / k_knn_bf16x3 / k_knn_rerank_cert
# --------------------------------------------------------------------------
def pad_dim(dim):
    return 128 if dim <= 128 else 192


def bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even, by bit arithmetic (finite x)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


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
    squares (lane l adds lane l ^ o for o = 1, 2, .. 32), then the chunks added
    in order to a sum that starts at 0; float32 throughout."""
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


def c_dp(dp):
    """DESIGN.md §10.1's table, written out."""
    return 2.0 * (3.0 * dp + 8.0) * 2.0 ** -23 + 2.0 ** -16 * (1.0 + 2.0 ** -6) + 2.0 ** -17


ABS_TERM = 2.0 ** -50
MAX_SUM = 2.0 ** 126


def norms64(rows):
    x = np.asarray(rows, dtype=np.float64)
    return (x * x).sum(axis=1)


def dist64(q, x):
    """float64 |q - x|^2, [nq][n]."""
    q = np.asarray(q, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    d = q[:, None, :] - x[None, :, :]
    return (d * d).sum(axis=2)


def oracle_dist(oracle, q, x):
    """L2Dist of every pair by the oracle, float32 [nq][n]."""
    return np.stack([oracle.l2_batch(np.ascontiguousarray(r), np.ascontiguousarray(x, dtype=F32)) for r in
                     np.ascontiguousarray(q, dtype=F32)])


def eps_bound(dp, qn64, xn64):
    return c_dp(dp) * (qn64 + xn64) + ABS_TERM


# --------------------------------------------------------------------------
# rows for the split and the norms
# --------------------------------------------------------------------------
def _from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(F32)


SPLIT_FAMILIES = ("normal", "mantissa24", "halfway_even", "halfway_odd", "zeros", "subnormal", "lo_subnormal")


def split_family(name, n, dim, seed=0):
    """n rows of one value family (SPLIT_FAMILIES)."""
    rng = np.random.default_rng([seed, dim, SPLIT_FAMILIES.index(name)])
    sign = rng.integers(0, 2, (n, dim), dtype=np.uint32) << np.uint32(31)
    mant = rng.integers(0, 1 << 23, (n, dim), dtype=np.uint32)
    if name == "normal":
        return rng.standard_normal((n, dim)).astype(F32)
    if name == "mantissa24":      # all 24 bits significant: the last mantissa bit set
        e = rng.integers(120, 135, (n, dim), dtype=np.uint32) << np.uint32(23)
        return _from_bits(sign | e | mant | np.uint32(1))
    if name in ("halfway_even", "halfway_odd"):   # exactly between two bf16 values; the lower one even / odd
        e = rng.integers(100, 150, (n, dim), dtype=np.uint32) << np.uint32(23)
        top = (mant & np.uint32(0x7E0000)) | (np.uint32(0x10000) if name == "halfway_odd" else np.uint32(0))
        return _from_bits(sign | e | top | np.uint32(0x8000))
    if name == "zeros":           # +0 and -0
        return _from_bits(sign)
    if name == "subnormal":       # f32 subnormals
        return _from_bits(sign | np.maximum(mant, np.uint32(1)))
    if name == "lo_subnormal":    # normal x < 2^-118: |x - hi| <= 2^-127, below bf16's smallest normal
        e = rng.integers(2, 9, (n, dim), dtype=np.uint32) << np.uint32(23)
        return _from_bits(sign | e | mant | np.uint32(1))
    raise ValueError(name)


def split_rows_mixed(dim, per_family=6, seed=0):
    """Every family, per_family rows each, family f in rows [f * per_family, ...)."""
    return np.concatenate([split_family(f, per_family, dim, seed) for f in SPLIT_FAMILIES])


# --------------------------------------------------------------------------
# (q, x) pairs for the prefilter error
# --------------------------------------------------------------------------
PREF_SCALES = {"scale_2^-70": -70, "scale_2^-25": -25, "scale_2^30": 30, "scale_2^58": 58}
PREF_FAMILIES = ("normal", "positive", "alternating", "near", "integer") + tuple(PREF_SCALES)
PREF_DIMS = (1, 8, 100, 128, 129, 192)
PREF_N, PREF_NQ = 64, 66   # every base row is a candidate; a second, ragged block of query rows


def _positive(rng, n, dim):   # [1, 2) with all 24 mantissa bits in use
    return _from_bits(np.uint32(0x3F800000) | rng.integers(0, 1 << 23, (n, dim), dtype=np.uint32) | np.uint32(1))


def pref_family(name, dim, seed=0):
    """(q [PREF_NQ][dim], x [PREF_N][dim]) of one value family."""
    rng = np.random.default_rng([seed, dim, PREF_FAMILIES.index(name)])
    n, nq = PREF_N, PREF_NQ
    if name == "normal" or name in PREF_SCALES:
        q = rng.standard_normal((nq, dim)).astype(F32)
        x = rng.standard_normal((n, dim)).astype(F32)
        if name in PREF_SCALES:   # a power of two: exact
            s = F32(2.0) ** F32(PREF_SCALES[name])
            q, x = q * s, x * s
        return q, x
    if name == "positive":
        return _positive(rng, nq, dim), _positive(rng, n, dim)
    if name == "alternating":     # every product q_i x_i changes sign with i
        alt = np.where(np.arange(dim) % 2 == 0, F32(1), F32(-1))
        return _positive(rng, nq, dim), _positive(rng, n, dim) * alt
    if name == "near":            # x_j = q_j moved by up to 4 ulps per coordinate
        q = rng.standard_normal((nq, dim)).astype(F32)
        x = q[:n].copy()
        x = (x.view(np.uint32) + rng.integers(0, 5, (n, dim), dtype=np.uint32)).view(F32)
        return q, x
    if name == "integer":
        return (rng.integers(0, 256, (nq, dim)).astype(F32), rng.integers(0, 256, (n, dim)).astype(F32))
    raise ValueError(name)


# --------------------------------------------------------------------------
# data with n > 64 (the certificate's premise, end-to-end edges)
# --------------------------------------------------------------------------
def clustered_floats(n, d, nq=0, centres=20, seed=11):
    """row i = centre[i % centres] + 0.1 N(0,1); queries = the centres of rows
    ::80 + 0.1 N(0,1)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d)).astype(F32)
    label = np.arange(n) % centres
    v = (c[label] + 0.1 * rng.standard_normal((n, d))).astype(F32)
    if not nq:
        return v
    ql = label[::80][:nq]
    q = (c[ql] + 0.1 * rng.standard_normal((len(ql), d))).astype(F32)
    return v, q


def near_duplicate_rows():
    """300 rows of dim 100, the first 100 within a few ulps of one row; four
    queries among them and five elsewhere."""
    rng = np.random.default_rng(5)
    n, d = 300, 100
    base = rng.standard_normal(d).astype(F32)
    v = rng.standard_normal((n, d)).astype(F32)
    for i in range(100):
        r = base.copy()
        r[i % 100] = r[i % 100] + F32(i) * np.spacing(r[i % 100])
        v[i] = r
    q = np.concatenate([v[[0, 3, 40, 99]], v[[120, 150, 200, 250, 299]] + F32(0.5)]).astype(F32)
    return v, q


SHAPE_N = (1, 63, 64, 65, 127, 128, 129, 193)
SHAPE_NQ = (1, 63, 64, 65, 130)
SHAPE_DIM = (1, 7, 8, 9, 127, 128, 129, 191, 192)
K_MID = 17   # the third k where no k <= 64 exceeds n


def shape_cases():
    """40 (n, nq, dim, k) cases: every (n, nq) pair once; along them dim walks
    its nine values and k its three (1, 64, and n + 1 where that is <= 64, else
    K_MID).  With 40 cases every pair of (n, nq), (n, k class), (nq, k class)
    and (dim, k class) occurs; (n, dim) has 72 pairs and (nq, dim) 45, more
    than 40 cases can hold, so 40 of each occur."""
    out = []
    for i, n in enumerate(SHAPE_N):
        for j, nq in enumerate(SHAPE_NQ):
            idx = i * len(SHAPE_NQ) + j
            kc = (j + 2 * (idx // 9)) % 3
            k = (1, 64, n + 1 if n + 1 < 64 else K_MID)[kc]
            out.append((n, nq, SHAPE_DIM[idx % 9], k, kc))
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


def descending_rows(integer):
    """(v [1024][128], q [1][128]): L2Dist(q, v_i) strictly decreases with i, so
    every tile of the prefilter inserts all its columns.  Floats: v_i = (2 -
    i / 1024) u for a fixed direction u, q = -u.  Integers: q = 0 and v_i has
    D = 1024 - i as 9 a + b: a coordinates of 3 and b of 1."""
    dim = 128
    if integer:
        v = np.zeros((DESC_N, dim), F32)
        for i in range(DESC_N):
            a, b = divmod(DESC_N - i, 9)
            v[i, :a] = 3
            v[i, a:a + b] = 1
        return v, np.zeros((1, dim), F32)
    u = np.random.default_rng(21).standard_normal(dim).astype(F32)
    s = (F32(2) - np.arange(DESC_N, dtype=F32) / F32(DESC_N))
    return (s[:, None] * u[None, :]).astype(F32), -u[None, :]


def identical_rows(integer, n=330, dim=24, copies=200, seed=3):
    """(v, q, ntie): `copies` identical rows in two runs (ids 10.. and the last
    ones), q[0:3] equal to them, q[3:] equal to other base rows; ntie = 3."""
    rng = np.random.default_rng([seed, int(integer)])
    gen = (lambda *s: rng.integers(0, 256, s).astype(F32)) if integer else (lambda *s: rng.standard_normal(s).astype(F32))
    v = gen(n, dim)
    row = gen(dim)
    v[10:10 + copies // 2] = row
    v[n - copies // 2:] = row
    q = np.stack([row, row, row, v[0], v[5], v[150], v[200]])
    return v, q, 3


def equidistant_rows(integer, n=600, seed=4):
    """(v, q, ntie): 200 rows at one exact non-zero L2Dist r^2 from q[0] = c:
    c +- r e_j for the 100 axes, the + rows at ids 0..99 (the first tiles), the
    - rows at the last 100 ids; the other rows are farther.  Integers: c in
    1..254, r = 1.  Floats: c in quarters, r = 0.5 (all sums exact)."""
    dim = 100
    rng = np.random.default_rng([seed, int(integer)])
    if integer:
        c = rng.integers(1, 255, dim).astype(F32)
        r = F32(1)
        v = rng.integers(0, 256, (n, dim)).astype(F32)
    else:
        c = (rng.integers(-8, 9, dim) / 4.0).astype(F32)
        r = F32(0.5)
        v = (c + rng.standard_normal((n, dim))).astype(F32)
    eye = np.eye(dim, dtype=F32) * r
    v[:100] = c + eye
    v[n - 100:] = c - eye
    q = np.stack([c, c])
    return v, q, 2


# --------------------------------------------------------------------------
# robustPrune
# --------------------------------------------------------------------------
def prune_trace(oracle, X, u, cand, m, alpha):
    """robustPrune's greedy pass restated over the oracle's L2Dist: (accepted,
    discarded, discards before the last accept).  Lists of at most m are kept."""
    X = np.ascontiguousarray(X, dtype=F32)
    cand = np.asarray(cand, dtype=np.uint32)
    if len(cand) <= m:
        return list(cand), [], 0
    d = oracle.l2_batch(X[u], X[cand])
    order = np.lexsort((np.arange(len(cand)), d.view(np.uint32)))
    acc, disc, before = [], [], 0
    for p in order:
        v = cand[p]
        ok = True
        if acc:
            da = oracle.l2_batch(X[v], X[np.array(acc, dtype=np.uint32)])
            ok = not bool(((da * F32(alpha)).astype(F32) < d[p]).any())
        if ok:
            acc.append(int(v))
            before = len(disc)
            if len(acc) == m:
                break
        else:
            disc.append(int(v))
    return acc, disc, before


def collinear_points(count, dim=8):
    """Vertex 0 at the origin and vertices 1..count at t e_0, t = 1 + i / 2048 <=
    3.01: the nearest is accepted and rejects every other one, (t - 1)^2 alpha <
    t^2, for alpha <= 2 (L2Dist is the squared distance)."""
    assert count <= 4120
    X = np.zeros((count + 1, dim), F32)
    X[1:, 0] = F32(1) + np.arange(count, dtype=F32) / F32(2048)
    return X


def late_rejector(dim=64):
    """(X, cand, w, j): vertex 0 at the origin, vertices 1..50 at (1 + i / 100)
    e_i, all accepted in that order (they lie far from each other), and w = 51
    at 1.355 e_35 (sorted right behind vertex 36 at 1.35 e_35), which only the 36th accepted one (list index j = 35, beyond a
    first round of 32) rejects.  With m = 42 the result is vertices 1..42."""
    X = np.zeros((52, dim), F32)
    for i in range(50):
        X[1 + i, i] = F32(1) + F32(i) / F32(100)
    X[51, 35] = 1.355
    cand = np.concatenate([np.arange(1, 41), [51], np.arange(41, 51)]).astype(np.uint32)
    return X, cand, 51, 35


def hub_discards(m=8, line=4100, dim=8):
    """collinear_points(line) plus m - 1 vertices far out on the other axes:
    after 1 accept and line - 1 discards (more than the kernel keeps) the far
    ones are accepted and complete the m."""
    X = np.concatenate([collinear_points(line, dim), np.zeros((m - 1, dim), F32)])
    for j in range(m - 1):
        X[line + 1 + j, 1 + j] = 10000.0
    cand = np.arange(1, line + m, dtype=np.uint32)
    return X, cand
