"""CPU: ``nomad_amd.triplets.create_triplets`` - the reference's triplet rule (src/utils/nsim_triplet_sampling.py:13-64) over
indices - on hand-written tables, ties included."""
import numpy as np
import pytest

from nomad_amd.triplets import create_triplets

# clip 0: spread values; clip 1: ties (0.9 twice, 0.5 twice); clip 2: conditions close to the clean clip's 1.0
TABLE = [[0.95, 0.80, 0.60, 0.35, 0.10, 0.97],
         [0.90, 0.90, 0.50, 0.50, 0.20, 0.70],
         [0.99, 0.98, 0.40, 0.30, 0.20, 0.10]]
C = 6


def _members(b):
    return np.array(TABLE[b] + [1.0])


def _check_rows(t, hard, full_pool):
    """Every returned row against the rule.  full_pool: N = 1, so each row was drawn from its clip's whole pool and "nearest" can be
    recomputed; with N > 1 a dropped draw also takes its anchor and positive out, so only what needs no pool is checked."""
    used = {}
    for b, a, p, n in zip(*(t[k].tolist() for k in ("clip", "anchor", "positive", "negative"))):
        v = _members(b)
        gone = used.setdefault(b, set())
        assert len({a, p, n}) == 3 and not {a, p, n} & gone, (b, a, p, n, gone)
        gone |= {a, p}
        dp, dn = abs(v[p] - v[a]), abs(v[n] - v[a])
        assert dp < dn
        if not hard:
            assert dn > dp + 0.05, "an easy negative is beyond the positive's distance plus the margin"
        if full_pool:
            others = [c for c in range(C + 1) if c != a]
            assert p == min(others, key=lambda c: (abs(v[c] - v[a]), c)), "the nearest member, ties to the lower index"
            if hard:
                rest = [c for c in others if c != p]
                assert n == min(rest, key=lambda c: (abs(v[c] - v[a]), c)), "the hard negative is the nearest remaining member"


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("N", [1, 3])
def test_rows_obey_the_rule(hard, N):
    kept = 0
    for seed in range(40):
        t, dropped = create_triplets(TABLE, N=N, hard_sampling=hard, margin=0.05, rng=seed)
        K = len(t["clip"])
        kept += K
        assert K + dropped == 3 * N and all(len(t[k]) == K for k in t)
        assert t["clip"].dtype == np.int64 and t["anc_pos_dist"].dtype == np.float64
        _check_rows(t, hard, N == 1)
        assert (t["anc_pos_dist"] < t["anc_neg_dist"]).all()
        for i in range(K):
            v = _members(t["clip"][i])
            assert t["anc_pos_dist"][i] == abs(v[t["positive"][i]] - v[t["anchor"][i]])
            assert t["anc_neg_dist"][i] == abs(v[t["negative"][i]] - v[t["anchor"][i]])
    assert kept > 40 * N, "most draws yield a row on this table"


def test_the_pool_shrinks_across_a_clips_draws():
    # 7 members: draws take 2 each -> pools of 7, 5, 3 and then 1: the fourth draw of a clip is always dropped
    for seed in range(8):
        t, dropped = create_triplets(TABLE, N=4, hard_sampling=True, rng=seed)
        assert dropped >= 3 and len(t["clip"]) + dropped == 12
        for b in range(3):
            rows = np.flatnonzero(t["clip"] == b)
            taken = np.concatenate([t["anchor"][rows], t["positive"][rows]])
            assert len(rows) <= 3 and len(set(taken.tolist())) == len(taken), "an anchor or positive was drawn twice"


def test_ties_are_dropped_and_counted_not_returned():
    # every value equal: the positive's and the negative's distance tie at 0 whatever is drawn
    t, dropped = create_triplets([[1.0, 1.0, 1.0, 1.0]], N=2, hard_sampling=True, rng=0)
    assert len(t["clip"]) == 0 and dropped == 2
    # an easy set that is empty: nothing lies beyond the positive's distance plus a margin of 2
    t, dropped = create_triplets(TABLE, N=3, hard_sampling=False, margin=2.0, rng=1)
    assert len(t["clip"]) == 0 and dropped == 9
    # a pool of two (C = 1): no rows and no exception; a NaN condition never enters the pool
    t, dropped = create_triplets([[0.5], [0.7]], N=3, rng=2)
    assert len(t["clip"]) == 0 and dropped == 6 and t["anc_neg_dist"].shape == (0,)
    t, dropped = create_triplets([[0.5, float("nan"), 0.7]], N=1, rng=3)
    assert len(t["clip"]) == 1 and dropped == 0 and 1 not in (t["anchor"][0], t["positive"][0], t["negative"][0])
    t, dropped = create_triplets([[0.5, float("nan")]], N=1, rng=3)
    assert len(t["clip"]) == 0 and dropped == 1


def test_the_same_seed_gives_the_same_table_and_names_follow_the_indices():
    names = [[f"clip{b}/cond{c}" for c in range(C)] + [f"CLEAN/clip{b}"] for b in range(3)]
    a, da = create_triplets(TABLE, names=names, N=3, hard_sampling=False, rng=5)
    b, db = create_triplets(TABLE, names=names, N=3, hard_sampling=False, rng=5)
    assert da == db and sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    other = [create_triplets(TABLE, N=3, hard_sampling=False, rng=s)[0] for s in range(6, 12)]
    assert any(not np.array_equal(o["anchor"], a["anchor"]) for o in other), "the seed does not reach the draws"
    for i in range(len(a["clip"])):
        assert a["Anchor"][i] == names[a["clip"][i]][a["anchor"][i]] and a["Negative"][i] == names[a["clip"][i]][a["negative"][i]]
    gen = np.random.default_rng(5)
    c, _ = create_triplets(TABLE, N=3, hard_sampling=False, rng=gen)
    assert np.array_equal(c["anchor"], a["anchor"]), "a Generator is used as it is"


def test_argument_errors():
    with pytest.raises(ValueError, match="table"):
        create_triplets([0.5, 0.6])
    with pytest.raises(ValueError, match="N must"):
        create_triplets(TABLE, N=0)
    with pytest.raises(ValueError, match="margin"):
        create_triplets(TABLE, margin=float("nan"))
    with pytest.raises(ValueError, match="names"):
        create_triplets(TABLE, names=[["a"] * C] * 3)


def test_the_config_key_is_checked_without_a_gpu():
    """``triplets_on_device`` needs ``pad_mode: exact``; the check runs before anything touches a GPU."""
    from nomad_amd.train import Training, check_triplets_on_device
    key = dict(clean="clean", valid_clean="valid", clip=[10, 40])
    cfg = dict(experiment_name="Training", checkpoint_path="seeded", train_bs=6, val_bs=6, triplets_on_device=key)
    assert check_triplets_on_device(dict(cfg, triplets_on_device=None), "batch") is None
    m = check_triplets_on_device(cfg, "exact")
    assert m["N"] == 3 and m["normalize"] == -23.0 and m["hard_sampling"] is False and m["sampling_margin"] == 0.05 and m["snr_db"] is None
    with pytest.raises(ValueError, match="requires pad_mode: exact"):
        Training(cfg)
    with pytest.raises(ValueError, match="requires pad_mode: exact"):
        Training(dict(cfg, pad_mode="batch"))
    for bad, msg in ((dict(key, snr=[5]), "unknown keys"), (dict(key, clean=None), "clean and valid_clean"),
                     (dict(clean="a", valid_clean="b"), "at least one of"), (dict(key, snr_db=[5]), "needs noise"), (dict(key, N=7), "at most train_bs")):
        with pytest.raises(ValueError, match=msg):
            check_triplets_on_device(dict(cfg, triplets_on_device=bad), "exact")
