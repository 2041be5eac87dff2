"""Timestep-loss definitions on the host: the bucket edges, the draw's arithmetic, the unbiasedness of the
loss-aware table, the Min-SNR weights and the argument checks.  No GPU: the draw and the table are tests/_tloss_ref.py's
restatement, which tests/test_gpu_tloss.py holds the kernels to bit for bit.

Bars (derived):
  * the 4096 grid points u0 = (i + 0.5) / 4096 that fall into an interval of length p number within 1 of 4096 p
    (grid points in an interval; the fp32 rounding of the grid points is exact: (2 i + 1) / 8192 with 2 i + 1 < 2^13);
  * unbiasedness: iw_tab is n_k / (T q_k) rounded to fp32, relative error <= 2^-24, so sum_t (q_k / n_k) iw_k f_t
    differs from mean_t f_t by at most 2^-24 mean|f| plus fp64 summation noise: 1e-6 relative for positive f.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import _tloss_ref as R
from cdm_amd.trainer import check_t_loss, min_snr_weights, t_bucket_edges, t_table
from cdm_amd.diffusion import Schedule

GRID = ((np.arange(4096, dtype=np.float64) + 0.5) / 4096).astype(np.float32)


@pytest.mark.parametrize("t_buckets", [1, 7, 64, 1024])
@pytest.mark.parametrize("T", [1, 7, 100, 1500])
def test_edges_partition_the_timesteps(T, t_buckets):
    NB, e = R.edges(T, t_buckets)
    assert NB == min(t_buckets, T) and e[0] == 0 and e[-1] == T and len(e) == NB + 1
    assert (np.diff(e) >= 1).all()
    owner = np.full(T + 1, -1)
    for k in range(NB):
        assert (owner[e[k] + 1:e[k + 1] + 1] == -1).all()
        owner[e[k] + 1:e[k + 1] + 1] = k
    assert (owner[1:] >= 0).all()
    assert [R.bucket_of(t, T, NB) for t in range(1, T + 1)] == owner[1:].tolist()
    assert np.array_equal(t_bucket_edges(T, NB), e)
    assert check_t_loss(None, 5.0, "uniform", t_buckets, 0.99, 10, 1e-3, T) == (None, NB)


@pytest.mark.parametrize("T,NB", [(1, 1), (7, 7), (1500, 64), (1500, 7)])
@pytest.mark.parametrize("name", ["warmup", "skewed", "zero_bucket"])
def test_draw_stays_in_range_at_u_equal_one(T, NB, name):
    cdf, iw_tab = R.three_tables(T, NB)[name]
    _, e = R.edges(T, NB)
    for u0, u1 in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (np.float32(2.0 ** -25), np.float32(1.0 - 2.0 ** -24))):
        t, iw, k = R.draw(np.array([u0, u1], np.float32), T, NB, cdf, iw_tab)
        assert 0 <= k[0] <= NB - 1 and e[k[0]] + 1 <= t[0] <= e[k[0] + 1]
        if u0 == 1.0:
            assert k[0] == NB - 1
        if u1 == 1.0:
            assert t[0] == e[k[0] + 1]


@pytest.mark.parametrize("name", ["warmup", "skewed", "zero_bucket"])
def test_draw_follows_the_table(name):
    T, NB = 1500, 64
    cdf, iw_tab = R.three_tables(T, NB)[name]
    u = np.stack([GRID, np.full(4096, 0.5, np.float32)], 1).reshape(-1)
    t, iw, k = R.draw(u, T, NB, cdf, iw_tab)
    counts = np.bincount(k, minlength=NB)
    p = np.diff(np.concatenate([[0.0], cdf]))
    p[-1] = 1.0 - cdf[-2]                                   # the last cdf entry is never consulted
    assert np.abs(counts - 4096 * p).max() < 1.0, np.abs(counts - 4096 * p).max()
    if name == "zero_bucket":
        assert counts[NB // 2] == 0
    assert np.array_equal(iw, iw_tab[k])


@pytest.mark.parametrize("T,NB", [(7, 7), (1500, 64), (1500, 7), (100, 3)])
def test_u1_reaches_every_timestep_of_its_bucket_and_no_other(T, NB):
    cdf, iw_tab = R.uniform_table(T, NB)
    _, e = R.edges(T, NB)
    for k in range(NB):
        lo = 0.0 if k == 0 else cdf[k - 1]
        u0 = np.float32(0.5 * (lo + cdf[k]))
        assert lo <= np.float64(u0) < cdf[k]
        u = np.stack([np.full(4096, u0, np.float32), GRID], 1).reshape(-1)
        t, _, kk = R.draw(u, T, NB, cdf, iw_tab)
        assert (kk == k).all()
        assert sorted(set(t.tolist())) == list(range(e[k] + 1, e[k + 1] + 1))


def _random_record(rng, NB, warm=True):
    rec = np.empty((NB, 3))
    rec[:, 0] = rng.integers(10 if warm else 0, 50, NB)
    rec[:, 1] = rng.random(NB)
    rec[:, 2] = 10.0 ** rng.uniform(-8, 2, NB)
    return rec


@pytest.mark.parametrize("T,NB", [(7, 7), (1500, 64), (1500, 7), (1500, 1024), (5, 1)])
def test_importance_weights_keep_the_objective_unbiased(T, NB):
    rng = np.random.default_rng(T * 31 + NB)
    _, e = R.edges(T, NB)
    nk = np.diff(e).astype(np.float64)
    kt = np.array([R.bucket_of(t, T, NB) for t in range(1, T + 1)])
    for trial in range(4):
        rec = _random_record(rng, NB)
        f = 10.0 ** rng.uniform(-3, 3, T)
        cdf, iw, q, uniform = R.table(rec, T, NB, 10, 1e-3)
        assert not uniform and abs(cdf[-1] - 1.0) < 1e-12 and (q > 0).all()
        est = np.sum((q[kt] / nk[kt]) * iw[kt].astype(np.float64) * f)
        assert abs(est - f.mean()) <= 1e-6 * f.mean()
        mine = t_table(rec, T, NB, 10, 1e-3)             # the package's host copy (t_loss_report) is the same table
        assert np.array_equal(mine[0], cdf) and np.array_equal(mine[1], iw) and np.array_equal(mine[2], q)
        rec[rng.integers(NB), 0] = 9                     # one bucket short of the warm-up: the uniform form, exactly
        cdf, iw, q, uniform = R.table(rec, T, NB, 10, 1e-3)
        assert uniform and (iw == 1.0).all() and cdf[-1] == 1.0
        assert np.array_equal(cdf, e[1:] / np.float64(T)) and np.array_equal(q, nk / np.float64(T))
        f_int = [int(v) for v in rng.integers(0, 1000, T)]      # in rationals: the bucket's n_k / T over its n_k
        est = sum(Fraction(int(nk[k]), T) / int(nk[k]) * int(iw[k]) * v for k, v in zip(kt, f_int))
        assert est == Fraction(sum(f_int), T)
        assert np.array_equal(t_table(rec, T, NB, 10, 1e-3)[0], cdf)


def test_all_zero_second_moment_gives_the_uniform_form():
    rec = np.zeros((7, 3))
    rec[:, 0] = 100
    cdf, iw, q, uniform = R.table(rec, 1500, 7, 10, 1e-3)
    assert uniform and (iw == 1.0).all()
    rec[3, 2] = np.inf
    assert R.table(rec, 1500, 7, 10, 1e-3)[3]


def test_record_update_restatement():
    T, NB, HW = 100, 4, 16
    rec = np.zeros((NB, 3))
    row_sq = np.array([16.0, 32.0, np.nan, 8.0])
    t = np.array([1, 2, 3, 100])
    out = R.record_update(rec, row_sq, t, None, HW, T, NB, 0.25)
    assert out[0].tolist() == [2.0, 1.0 + 0.25 * (2.0 - 1.0), 1.0 + 0.25 * (4.0 - 1.0)]
    assert out[3].tolist() == [1.0, 0.5, 0.25] and not out[1:3].any()


def test_min_snr_weights():
    T, gamma = 1500, 5.0
    ab = Schedule(T, "cpu").ab_t
    w = min_snr_weights(ab, gamma)
    assert w.dtype == torch.float32 and tuple(w.shape) == (T + 1,) and float(w[0]) == 0.0
    ab64 = ab.double().numpy()[1:]
    snr = ab64 / ((1.0 - ab64) * (1.0 - ab64))
    want = np.minimum(1.0, gamma / snr).astype(np.float32)
    assert np.array_equal(w.numpy()[1:], want)
    assert (w <= 1).all() and (w.numpy()[1:][snr <= gamma] == 1.0).all() and (w.numpy()[1:][snr > gamma] < 1.0).all()
    assert (np.diff(w.numpy()[1:]) >= 0).all(), "non-decreasing in t"
    assert 0 < int((w == 1).sum()) < T
    table, NB = check_t_loss("min_snr", gamma, "loss", 64, 0.99, 10, 1e-3, T)
    assert torch.equal(table, w) and NB == 64
    assert not torch.equal(min_snr_weights(ab, 1.0), w)


def test_argument_checks():
    T = 100
    ok = dict(loss_weight=None, snr_gamma=5.0, t_sampler="uniform", t_buckets=64, t_ema=0.99, t_warmup=10, t_mix=1e-3)

    def bad(**kw):
        a = {**ok, **kw}
        with pytest.raises(ValueError):
            check_t_loss(a["loss_weight"], a["snr_gamma"], a["t_sampler"], a["t_buckets"], a["t_ema"], a["t_warmup"],
                         a["t_mix"], T)
    bad(loss_weight="snr"); bad(t_sampler="importance")
    bad(loss_weight=np.ones(T)); bad(loss_weight=np.ones(T + 2)); bad(loss_weight=np.ones((T + 1, 1)))
    for v in (-1.0, float("nan"), float("inf")):
        tab = np.ones(T + 1); tab[5] = v
        bad(loss_weight=tab)
    for g in (0.0, -1.0, float("nan")):
        bad(snr_gamma=g)
        with pytest.raises(ValueError):
            min_snr_weights(Schedule(T, "cpu").ab_t, g)
    bad(t_buckets=0); bad(t_buckets=1025); bad(t_buckets=2.5)
    bad(t_ema=1.0); bad(t_ema=-0.1); bad(t_ema=float("nan"))
    bad(t_warmup=0); bad(t_mix=0.0); bad(t_mix=1.5); bad(t_mix=float("nan"))
    tab = np.ones(T + 1); tab[0] = float("nan")             # entry 0 is ignored
    w, NB = check_t_loss(tab, 5.0, "loss", 1024, 0.0, 1, 1.0, T)
    assert NB == T and float(w[0]) == 0.0 and (w[1:] == 1).all()


def test_trainer_rejects_bad_options_before_it_touches_the_model():
    from cdm_amd import Trainer
    for kw in ({"t_sampler": "importance"}, {"loss_weight": "snr"}, {"t_buckets": 0}, {"t_ema": 1.0}, {"t_warmup": 0},
               {"t_mix": 0.0}, {"snr_gamma": 0.0}, {"loss_weight": [1.0, 2.0]}):
        with pytest.raises(ValueError):
            Trainer(None, 1e-3, 100, 4, **kw)                # model None: anything past the checks would fail otherwise
