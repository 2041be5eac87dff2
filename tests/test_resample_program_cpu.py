"""The position program of resampling / late start and the per-position table builders: pure host functions, no GPU.
The definition is tests/_resample_ref.py."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
import _ddim_ref as D
import _resample_ref as RS

T = 100


def _ab():
    return R.make_schedule(T)[2]


def _mod():
    from cdm_amd import diffusion
    return diffusion


def _triples(prog):
    return [(int(prog.from_t[p]), int(prog.land_t[p]), int(prog.up_t[p])) for p in range(prog.P, 0, -1)]


def test_walk_written_out_by_hand():
    """S = 12, J = 3, R = 2 on uniform(100, 12).  State indices, a jump at each '->':
    12 11 10 9 -> 12 11 10 9 8 7 6 -> 9 8 7 6 5 4 3 -> 6 5 4 3 2 1 0: 21 positions."""
    m = _mod()
    taus = m.timestep_subsequence(T, 12)
    assert taus == [8, 17, 25, 33, 42, 50, 58, 67, 75, 83, 92, 100]
    expect = [
        (100, 92, 92), (92, 83, 83), (83, 75, 100),                                   # 12 11 10 -> 9, jump to 12
        (100, 92, 92), (92, 83, 83), (83, 75, 75), (75, 67, 67), (67, 58, 58), (58, 50, 75),     # ... 6, jump to 9
        (75, 67, 67), (67, 58, 58), (58, 50, 50), (50, 42, 42), (42, 33, 33), (33, 25, 50),      # ... 3, jump to 6
        (50, 42, 42), (42, 33, 33), (33, 25, 25), (25, 17, 17), (17, 8, 8), (8, 0, 0),
    ]
    prog = m.resample_program(_ab(), taus, jump=3, resamples=2)
    assert prog.P == 21 and _triples(prog) == expect
    assert RS.program(taus, 3, 2) == expect
    for v in prog:
        assert v.shape == (22,)
    assert prog.from_t.dtype == np.int32 and prog.fa.dtype == np.float32 and prog.fb.dtype == np.float32
    assert (prog.from_t[0], prog.land_t[0], prog.up_t[0], prog.fa[0], prog.fb[0]) == (0, 0, 0, 1.0, 0.0)


@pytest.mark.parametrize("S", [1, 2, 5, 12, 13, 30])
@pytest.mark.parametrize("J", [1, 2, 3, 5])
@pytest.mark.parametrize("R_", [1, 2, 4])
def test_position_count(S, J, R_):
    """P = S' + (R - 1) J (S' // J - 1); ValueError when R > 1 and there is no jump point; the walk is the
    restatement's; it ends on 0 and every position descends."""
    m = _mod()
    taus = m.timestep_subsequence(T, S)
    if R_ > 1 and S < 2 * J:
        with pytest.raises(ValueError, match="jump point"):
            m.resample_program(_ab(), taus, J, R_)
        return
    prog = m.resample_program(_ab(), taus, J, R_)
    assert prog.P == S + (R_ - 1) * J * (S // J - 1 if S >= 2 * J else 0)
    tr = _triples(prog)
    assert tr == RS.program(taus, J, R_)
    assert tr[0][0] == T and tr[-1][1] == 0 and all(j < i and u >= j for i, j, u in tr)
    assert all(a[2] == b[0] for a, b in zip(tr, tr[1:]))          # each position starts where the last one left the state
    assert sum(u != j for _, j, u in tr) == (R_ - 1) * (S // J - 1 if S >= 2 * J else 0)


@pytest.mark.parametrize("S,spacing", [(12, "uniform"), (7, "quadratic"), (1, "uniform"), (2, "uniform"), (100, "uniform")])
def test_plain_program_reproduces_the_tables_bit_for_bit(S, spacing):
    """R = 1, no t_start: the program is the plain walk and the builders from pairs give ddim_tables / dpmpp_tables."""
    m = _mod()
    ab = _ab()
    taus = m.timestep_subsequence(T, S, spacing)
    prog = m.resample_program(ab, taus)
    assert prog.P == S and list(prog.from_t[1:]) == taus and list(prog.land_t[1:]) == [0] + taus[:-1]
    assert np.array_equal(prog.up_t, prog.land_t)
    for eta in (0.0, 0.5, 1.0):
        for a, b in zip(m.ddim_tables(ab, taus, eta), m.ddim_tables_from_pairs(ab, prog.from_t, prog.land_t, eta)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    for order in (1, 2):
        for dt in (np.float32, np.float64):
            got = m.dpmpp_tables_from_pairs(ab, prog.from_t, prog.land_t, prog.up_t, order, dt)
            for a, b in zip(m.dpmpp_tables(ab, taus, order, dt), got):
                assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("J,R_,t_start", [(3, 2, None), (2, 3, None), (1, 2, None), (2, 2, 60)])
def test_tables_of_a_program(J, R_, t_start):
    """c1 == 0 exactly at the first position, after a jump, where the position lands on 0; fa == 1 and fb == 0 exactly
    where there is no jump, fa^2 + fb^2 = 1 to fp32 rounding elsewhere; every table equals the restatement's python-float
    value to one fp32 ulp (numpy's and libm's log may differ in the last fp64 bit before the single rounding)."""
    m = _mod()
    ab = _ab()
    taus = m.timestep_subsequence(T, 12)
    prog = m.resample_program(ab, taus, J, R_, t_start)
    tr = RS.program(taus, J, R_, t_start)
    assert _triples(prog) == tr
    Pn = prog.P
    sq, ra, c0, c1, cx, cd = m.dpmpp_tables_from_pairs(ab, prog.from_t, prog.land_t, prog.up_t, 2)
    for q, (i, j, u) in enumerate(tr):
        p = Pn - q
        first_order = q == 0 or tr[q - 1][2] != tr[q - 1][1] or j == 0
        assert (c1[p] == 0) == first_order, p
        assert (c0[p] == 1) == first_order, p
        if u == j:
            assert prog.fa[p] == 1.0 and prog.fb[p] == 0.0
        else:
            assert 0 < prog.fa[p] < 1 and 0 < prog.fb[p] < 1
            assert abs(float(prog.fa[p]) ** 2 + float(prog.fb[p]) ** 2 - 1) <= 4 * 2.0 ** -24
    assert sum(c1 != 0) > 0
    o1 = m.dpmpp_tables_from_pairs(ab, prog.from_t, prog.land_t, prog.up_t, 1)
    assert (o1[3] == 0).all() and (o1[2] == 1).all()

    def close(mine, ref):
        ref = ref.numpy()[::-1]
        assert np.all(np.abs(mine[1:] - ref) <= np.spacing(np.abs(ref)).astype(np.float32)), (mine[1:], ref)
    for mine, ref in zip((prog.fa, prog.fb), RS.jump_coefficients(ab, tr)):
        close(mine, ref)
    for mine, ref in zip((sq, ra, c0, c1, cx, cd), RS.dpmpp_coefficients(ab, tr, 2)):
        close(mine, ref)
    for eta in (0.0, 1.0):
        for mine, ref in zip(m.ddim_tables_from_pairs(ab, prog.from_t, prog.land_t, eta), RS.ddim_coefficients(ab, tr, eta)):
            close(mine, ref)


def test_truncation_by_t_start():
    m = _mod()
    ab = _ab()
    taus = m.timestep_subsequence(T, 12)
    for t_start, kept in ((100, 12), (99, 11), (60, 7), (58, 7), (57, 6), (8, 1)):
        prog = m.resample_program(ab, taus, t_start=t_start)
        assert prog.P == kept and list(prog.from_t[1:]) == taus[:kept]
        assert int(prog.from_t[-1]) == max(t for t in taus if t <= t_start)
        assert np.array_equal(prog.up_t, prog.land_t) and (prog.fb == 0).all()
    prog = m.resample_program(ab, taus, jump=3, resamples=2, t_start=60)       # S' = 7: jump points 3 (6 > 7 - 3)
    assert prog.P == 7 + 3 and _triples(prog) == RS.program(taus, 3, 2, 60)
    assert [u for _, j, u in _triples(prog) if u != j] == [taus[5]]
    assert torch.is_tensor(ab) and m.resample_program(ab.numpy(), taus, t_start=60).P == 7


def test_value_errors():
    m = _mod()
    ab = _ab()
    taus = m.timestep_subsequence(T, 12)
    for kw in (dict(t_start=0), dict(t_start=T + 1), dict(t_start=-3), dict(t_start=7), dict(t_start=50.5),
               dict(jump=0), dict(jump=-1), dict(jump=1.5), dict(jump=True), dict(resamples=0), dict(resamples=2.0),
               dict(resamples=2, jump=7), dict(resamples=3, jump=4, t_start=60)):
        with pytest.raises(ValueError):
            m.resample_program(ab, taus, **kw)
    for bad in ([], [0, 50, 100], [50, 40, 100], [10, 50]):
        with pytest.raises(ValueError):
            m.resample_program(ab, bad)
    prog = m.resample_program(ab, taus, 3, 2)
    with pytest.raises(ValueError):
        m.ddim_tables_from_pairs(ab, prog.from_t, prog.land_t, eta=-1.0)
    with pytest.raises(ValueError):
        m.ddim_tables_from_pairs(ab, prog.land_t, prog.from_t)               # ascending pairs
    with pytest.raises(ValueError):
        m.ddim_tables_from_pairs(ab, prog.from_t, prog.land_t[:-1])
    with pytest.raises(ValueError):
        m.dpmpp_tables_from_pairs(ab, prog.from_t, prog.land_t, prog.up_t, order=3)
    with pytest.raises(ValueError):
        m.dpmpp_tables_from_pairs(ab, prog.from_t + T, prog.land_t, prog.up_t)
    assert D.subsequence(T, 12) == taus
