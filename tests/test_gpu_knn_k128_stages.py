"""The stages of pm_knn_k128 through pm_knn_stages_k128: the
prefilter distances are the 64-key kernels' bit for bit, within the bound eps
the certificate relies on; the certificate's premise with 128 keys on data with
more than 128 base rows; and the uncertified rows against pm_knn_stages_wide's."""
import numpy as np
import pytest

from tests import knn_k128_ref as K

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", [1, 100, 128, 192, 193, 512, 1024])
@pytest.mark.parametrize("family", ["normal", "alternating"])
def test_prefilter_bits_equal_the_64_key_kernels(ctx, family, dim):
    """n = 64: every base row is a candidate of both lists, so the sorted (id,
    prefilter distance bits) keys of pm_knn_stages_k128 are pm_knn_stages_wide's
    and the other 64 slots are empty; so are the split rows and the norms."""
    import pacmann_amd as pm
    q, x = K.pref_family(family, dim)
    assert len(x) == 64
    a = pm.knn_stages_k128(x, q, 1, ctx)
    b = pm.knn_stages_wide(x, q, 1, ctx)
    assert a["dp"] == b["dp"] == K.pad_dim(dim)
    assert a["cand"].shape == a["pref"].shape == (len(q), K.TOP)
    assert (np.sort(b["cand"], axis=1) == np.arange(64, dtype=np.uint32)).all()
    assert np.array_equal(a["cand"][:, :64], b["cand"])
    assert np.array_equal(bits(a["pref"][:, :64]), bits(b["pref"]))
    assert (a["cand"][:, 64:] == K.EMPTY).all() and (bits(a["pref"][:, 64:]) == K.EMPTY).all()
    for name in ("bhi", "blo", "qnorm", "bnorm"):
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
    assert a["maxnorm"] == b["maxnorm"]
    assert (bits(a["eps"]) == K.EMPTY).all() and len(a["uncertified"]) == 0   # n <= 128: no row judged


@pytest.mark.parametrize("dim", [100, 320])
def test_prefilter_error_within_eps_at_128_rows(ctx, oracle, dim):
    """n = 128: every base row is a candidate once, in both halves of the list;
    |prefilter distance - L2Dist| <= c_dp (|q|^2 + |x|^2) + 2^-50 for every
    pair, against the oracle."""
    import pacmann_amd as pm
    rng = np.random.default_rng([17, dim])
    x = rng.standard_normal((128, dim)).astype(np.float32)
    q = rng.standard_normal((66, dim)).astype(np.float32)
    s = pm.knn_stages_k128(x, q, 1, ctx)
    cand, pref = s["cand"], s["pref"]
    assert (np.sort(cand, axis=1) == np.arange(128, dtype=np.uint32)).all()
    keys = (bits(pref).astype(np.uint64) << np.uint64(32)) | cand
    assert (keys[:, 1:] > keys[:, :-1]).all()
    by_id = np.empty((len(q), 128), np.float32)
    np.put_along_axis(by_id, cand.astype(np.int64), pref, axis=1)
    bound = K.eps_bound(s["dp"], K.norms64(q)[:, None], K.norms64(x)[None, :])
    r = np.abs(by_id.astype(np.float64) - K.oracle_dist(oracle, q, x).astype(np.float64)) / bound
    print(f"PREFILTER_SLACK_K128 dp={s['dp']} dim={dim} max_err_over_bound oracle={r.max():.4f}")
    assert r.max() <= 1.0
    assert (bits(s["eps"]) == K.EMPTY).all() and len(s["uncertified"]) == 0


@pytest.fixture(scope="module", params=[100, 192, 320, 768])
def premise(request, oracle):
    v, q = K.clustered_floats(1000, request.param, nq=50)
    od_all = K.oracle_dist(oracle, q, v)
    oi, od = oracle.knn(v, q, K.TOP)
    return v, q, od_all, oi, od


def test_certificate_premise(ctx, premise):
    """n > 128: the keys are strictly ascending, tau is the 128th prefilter
    distance, no base row outside the 128 lies more than the row's eps below tau,
    and that eps is at least the derived bound."""
    import pacmann_amd as pm
    v, q, od_all, _, _ = premise
    s = pm.knn_stages_k128(v, q, 10, ctx)
    cand, pref = s["cand"], s["pref"]
    assert s["dp"] == K.pad_dim(v.shape[1]) and cand.shape == (len(q), K.TOP)
    assert (cand < len(v)).all() and (pref >= 0).all()
    keys = (bits(pref).astype(np.uint64) << np.uint64(32)) | cand
    assert (keys[:, 1:] > keys[:, :-1]).all()
    assert np.array_equal(bits(s["tau"]), bits(pref[:, K.TOP - 1]))
    tau, eps = s["tau"].astype(np.float64), s["eps"].astype(np.float64)
    assert np.isfinite(eps).all()
    assert (eps >= K.eps_bound(s["dp"], K.norms64(q), K.norms64(v).max())).all()
    slack = []
    for r in range(len(q)):
        outside = np.ones(len(v), bool)
        outside[cand[r]] = False
        assert outside.sum() == len(v) - K.TOP
        d = od_all[r, outside].astype(np.float64)
        assert (d >= tau[r] - eps[r]).all(), (r, d.min(), tau[r], eps[r])
        slack.append((tau[r] - d.min()) / eps[r])
        assert (np.abs(pref[r].astype(np.float64) - od_all[r, cand[r]]) <= eps[r]).all()
    print(f"PREMISE_K128 n={len(v)} dim={v.shape[1]}: max (tau - nearest outside) / eps = {max(slack):.4f}")


@pytest.mark.parametrize("k", [1, 10, 64, 100, 128])
def test_uncertified_rows(ctx, premise, k):
    """The uncertified list is exactly the rows for which dK < tau - eps fails in
    float64, its length is pm_knn_k128's fallback_rows, and the results are the
    oracle's either way."""
    import pacmann_amd as pm
    v, q, _, oi, od = premise
    s = pm.knn_stages_k128(v, q, k, ctx)
    dk = od[:, k - 1].astype(np.float64)
    fails = ~(dk < s["tau"].astype(np.float64) - s["eps"].astype(np.float64))
    assert s["uncertified"].tolist() == np.flatnonzero(fails).tolist()
    gi, gd, fb = pm.knn_k128(v, q, k, ctx, with_dist=True)
    assert fb == len(s["uncertified"])
    assert np.array_equal(gi, oi[:, :k]) and np.array_equal(bits(gd), bits(od[:, :k]))
    print(f"UNCERTIFIED_K128 n={len(v)} dim={v.shape[1]} k={k}: {fb} of {len(q)}")


def subset_data(name):
    kind, dim = name.split("_")
    if kind == "clustered":
        return K.clustered_floats(1000, int(dim), nq=50) + (0,)
    return K.near_tie_rows(int(dim))


@pytest.mark.parametrize("k", [10, 48, 64])
@pytest.mark.parametrize("name", ["clustered_100", "clustered_320", "neartie_100", "neartie_320"])
def test_uncertified_rows_are_a_subset_of_the_64_key_list(ctx, oracle, name, k):
    """The same data through both lists: tau_128 >= tau_64 at the same eps, so the
    rows 128 keys leave uncertified are among those 64 keys leave.  On the
    near-tie rows the float64 verdict (knn_k128_ref.subset_verdict) makes the
    subset strict at k = 48: the near-duplicate queries are on the 64-key list
    and not on the 128-key one."""
    import pacmann_amd as pm
    v, q, ntie = subset_data(name)
    a = pm.knn_stages_k128(v, q, k, ctx)
    b = pm.knn_stages_wide(v, q, k, ctx)
    assert np.array_equal(bits(a["eps"]), bits(b["eps"]))
    assert (a["tau"] >= b["tau"]).all()
    ua, ub = set(a["uncertified"].tolist()), set(b["uncertified"].tolist())
    print(f"SUBSET {name} k={k}: 128 keys {len(ua)}, 64 keys {len(ub)} of {len(q)}")
    assert ua <= ub
    if ntie and k == 48:
        sure64, sure128 = K.subset_verdict(oracle, v, q, k)
        assert sure64[:ntie].all() and sure128.all()
        assert set(range(ntie)) <= ub and not ua
        assert ua < ub
