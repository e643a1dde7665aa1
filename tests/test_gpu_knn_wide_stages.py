"""The stages of pm_knn_wide against the plain reference (tests/knn_wide_ref.py),
through pm_knn_stages_wide: the bf16 split and the norms at the wide dp bit for
bit, the measured error of the K-chunked three-product prefilter against the
bound eps the certificate relies on (DESIGN.md §10.1's table with the larger
dp, §10.2), and the certificate's premise on data with more than 64 base rows."""
import numpy as np
import pytest

from tests import knn_wide_ref as W

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", [193, 256, 1024])
def test_split_and_norms_bit_for_bit(ctx, dim):
    """hi, lo, the padding, the norms in the kernel's fixed order and the bits of
    the largest norm, on every value family; as base rows and as query rows."""
    import pacmann_amd as pm
    rows = W.split_rows_mixed(dim)
    n = len(rows)
    assert n <= 64
    s = pm.knn_stages_wide(rows, rows, 1, ctx)
    hi, lo = W.split_rows(rows)
    assert s["dp"] == W.pad_dim(dim) and s["bhi"].shape == hi.shape
    fam = np.repeat(np.array(W.SPLIT_FAMILIES), n // len(W.SPLIT_FAMILIES))
    for name, got, want in (("hi", s["bhi"], hi), ("lo", s["blo"], lo)):
        bad = np.argwhere(got != want)
        assert not len(bad), (name, fam[bad[0][0]], bad[0].tolist(), hex(got[tuple(bad[0])]), hex(want[tuple(bad[0])]))
        assert (got[:, dim:] == 0).all()
    norms = W.norms_fixed_order(rows)
    for name in ("bnorm", "qnorm"):
        bad = np.flatnonzero(bits(s[name]) != bits(norms))
        assert not len(bad), (name, fam[bad[0]], float(s[name][bad[0]]), float(norms[bad[0]]))
    assert s["maxnorm"] == int(bits(norms).max())


def pref_by_id(s, n):
    """The probe's prefilter distances as [nq][n] by base id (n <= 64: every base
    row is a candidate, once)."""
    cand, pref = s["cand"], s["pref"]
    assert (np.sort(cand[:, :n], axis=1) == np.arange(n, dtype=np.uint32)).all()
    assert (cand[:, n:] == W.EMPTY).all() and (bits(pref[:, n:]) == W.EMPTY).all()
    out = np.empty((len(cand), n), np.float32)
    np.put_along_axis(out, cand[:, :n].astype(np.int64), pref[:, :n], axis=1)
    return out


@pytest.mark.parametrize("dim", [193, 512, 1024])
@pytest.mark.parametrize("family", W.PREF_FAMILIES)
def test_prefilter_error_within_eps(ctx, oracle, family, dim):
    """|prefilter distance - L2Dist| <= c_dp (|q|^2 + |x|^2) + 2^-50 for every
    (q, x) pair, against the oracle's L2Dist and against the float64 distance:
    the bound of DESIGN.md §10.1's table at the wide dp.  Prints the largest
    error / bound."""
    import pacmann_amd as pm
    q, x = W.pref_family(family, dim)
    dp = W.pad_dim(dim)
    s = pm.knn_stages_wide(x, q, 1, ctx)
    assert s["dp"] == dp
    pref = pref_by_id(s, len(x)).astype(np.float64)
    assert np.isfinite(pref).all() and (pref >= 0).all()
    bound = W.eps_bound(dp, W.norms64(q)[:, None], W.norms64(x)[None, :])
    d_or = W.oracle_dist(oracle, q, x)
    r_or = np.abs(pref - d_or.astype(np.float64)) / bound
    r_64 = np.abs(pref - W.dist64(q, x)) / bound
    i, j = np.unravel_index(np.argmax(r_or), r_or.shape)
    print(f"PREFILTER_SLACK_W dp={dp} dim={dim} family={family} max_err_over_bound oracle={r_or.max():.4f} "
          f"float64={r_64.max():.4f} (pair q{i} x{j}: pref {pref[i, j]!r} L2Dist {float(d_or[i, j])!r} bound {bound[i, j]!r})")
    assert r_or.max() <= 1.0, (i, j)
    assert r_64.max() <= 1.0


@pytest.fixture(scope="module", params=[320, 768])
def premise(request, oracle):
    v, q = W.clustered_floats(1000, request.param, nq=50)
    od_all = W.oracle_dist(oracle, q, v)
    oi, od = oracle.knn(v, q, 64)
    return v, q, od_all, oi, od


def test_certificate_premise(ctx, premise):
    """n > 64: the keys are strictly ascending, tau is the 64th prefilter
    distance, no base row outside the 64 lies more than the row's eps below tau,
    and that eps is at least the derived bound."""
    import pacmann_amd as pm
    v, q, od_all, _, _ = premise
    s = pm.knn_stages_wide(v, q, 10, ctx)
    cand, pref = s["cand"], s["pref"]
    assert s["dp"] == W.pad_dim(v.shape[1])
    assert (cand < len(v)).all() and (pref >= 0).all()
    keys = (bits(pref).astype(np.uint64) << np.uint64(32)) | cand
    assert (keys[:, 1:] > keys[:, :-1]).all()
    assert np.array_equal(bits(s["tau"]), bits(pref[:, 63]))
    tau, eps = s["tau"].astype(np.float64), s["eps"].astype(np.float64)
    assert np.isfinite(eps).all()
    qn, xn = W.norms64(q), W.norms64(v)
    assert (eps >= W.eps_bound(s["dp"], qn, xn.max())).all()
    assert s["maxnorm"] == int(bits(s["bnorm"]).max())
    slack = []
    for r in range(len(q)):
        outside = np.ones(len(v), bool)
        outside[cand[r]] = False
        assert outside.sum() == len(v) - 64
        d = od_all[r, outside].astype(np.float64)
        assert (d >= tau[r] - eps[r]).all(), (r, d.min(), tau[r], eps[r])
        slack.append((tau[r] - d.min()) / eps[r])
        assert (np.abs(pref[r].astype(np.float64) - od_all[r, cand[r]]) <= eps[r]).all()
    print(f"PREMISE_W n={len(v)} dim={v.shape[1]}: max (tau - nearest outside) / eps = {max(slack):.4f}")


@pytest.mark.parametrize("k", [1, 10, 64])
def test_uncertified_rows(ctx, premise, k):
    """The uncertified list is exactly the rows for which dK < tau - eps fails in
    float64, its length is pm_knn_wide's fallback_rows, and the results are the
    oracle's either way."""
    import pacmann_amd as pm
    v, q, _, oi, od = premise
    s = pm.knn_stages_wide(v, q, k, ctx)
    dk = od[:, k - 1].astype(np.float64)
    fails = ~(dk < s["tau"].astype(np.float64) - s["eps"].astype(np.float64))
    assert s["uncertified"].tolist() == np.flatnonzero(fails).tolist()
    gi, gd, fb = pm.knn_wide(v, q, k, ctx, with_dist=True)
    assert fb == len(s["uncertified"])
    assert np.array_equal(gi, oi[:, :k]) and np.array_equal(bits(gd), bits(od[:, :k]))
    print(f"UNCERTIFIED_W n={len(v)} dim={v.shape[1]} k={k}: {fb} of {len(q)}")
