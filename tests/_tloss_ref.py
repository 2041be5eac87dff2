"""numpy restatement of the timestep-loss kernels (csrc/tloss.hip): the bucket edges, the draw from given
uniforms, the finalize of cdm_mse_weighted from given row sums, the record update and the table rebuild.  fp64 with one
operation per step, in the kernels' order, and fp32 where the kernels round; written from the header's contract, not
from the package's host code (trainer.t_table is checked against it in tests/test_tloss_cpu.py)."""
import numpy as np

F32, F64 = np.float32, np.float64


def edges(T, t_buckets):
    """(NB, edges [NB + 1]): NB = min(t_buckets, T), edge_k = (k T) // NB."""
    NB = min(int(t_buckets), int(T))
    return NB, np.array([(k * int(T)) // NB for k in range(NB + 1)], dtype=np.int64)


def bucket_of(t, T, NB):
    return (int(t) * int(NB) - 1) // int(T)


def uniform_table(T, NB):
    _, e = edges(T, NB)
    return e[1:].astype(F64) / F64(T), np.ones(NB, F32)


def draw(u, T, NB, cdf, iw_tab):
    """(t [B] int32, iw [B] fp32, k [B]) from u [2 B] fp32 (u0 = u[2b], u1 = u[2b + 1])."""
    _, e = edges(T, NB)
    u = np.asarray(u, dtype=F32)
    B = u.size // 2
    t, iw, ks = np.empty(B, np.int32), np.empty(B, F32), np.empty(B, np.int64)
    for b in range(B):
        u0, u1 = u[2 * b], u[2 * b + 1]
        k = int(np.sum(np.asarray(cdf[:NB - 1], dtype=F64) <= F64(u0)))
        nk = int(e[k + 1] - e[k])
        j = int(F32(nk) * u1)                       # fp32 product, truncated
        t[b] = e[k] + 1 + min(nk - 1, j)
        iw[b] = iw_tab[k]
        ks[b] = k
    return t, iw, ks


def omega(t, w_tab, iw, B):
    """omega [B] fp32: w_tab[t_b] * iw[b], one fp32 product; an absent table is 1."""
    w = np.ones(B, F32) if w_tab is None else np.asarray(w_tab, dtype=F32)[np.asarray(t)]
    i = np.ones(B, F32) if iw is None else np.asarray(iw, dtype=F32)
    return (w * i).astype(F32)


def finalize(row_sq, row_g, HW, om):
    """(loss fp32, dbias fp32) from the row sums (fp64) and omega (fp32)."""
    a, g = F64(0.0), F64(0.0)
    for b in range(len(row_sq)):
        a = a + F64(om[b]) * F64(row_sq[b])
        g = g + F64(row_g[b])
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(a / (F64(len(row_sq)) * F64(HW))), F32(g)


def record_update(rec, row_sq, t, w_tab, HW, T, NB, alpha):
    """rec [NB, 3] fp64 after one call (a copy)."""
    rec = np.array(rec, dtype=F64)
    alpha = F64(alpha)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(len(row_sq)):
            l = F64(row_sq[b]) / F64(HW)
            tb = int(t[b])
            if not np.isfinite(l) or tb < 1 or tb > T:
                continue
            k = bucket_of(tb, T, NB)
            wl = l if w_tab is None else F64(F32(w_tab[tb])) * l
            y = wl * wl
            n, m1, m2 = rec[k]
            if n == 0:
                rec[k, 1], rec[k, 2] = l, y
            else:
                rec[k, 1] = m1 + alpha * (l - m1)
                rec[k, 2] = m2 + alpha * (y - m2)
            rec[k, 0] = n + F64(1.0)
    return rec


def table(rec, T, NB, warmup, mix):
    """(cdf [NB] fp64, iw_tab [NB] fp32, q [NB] fp64, uniform?) from the record alone."""
    _, e = edges(T, NB)
    rec = np.asarray(rec, dtype=F64)
    S = F64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(NB):
            S = S + np.sqrt(rec[k, 2])
    nk = np.diff(e).astype(F64)
    if rec[:, 0].min() < warmup or not np.isfinite(S) or not S > 0:
        cdf, iw = uniform_table(T, NB)
        return cdf, iw, nk / F64(T), True
    mix, dT = F64(mix), F64(T)
    omm = F64(1.0) - mix
    cdf, iw, q = np.empty(NB, F64), np.empty(NB, F32), np.empty(NB, F64)
    run = F64(0.0)
    for k in range(NB):
        p1 = (omm * np.sqrt(rec[k, 2])) / S
        p2 = (mix * nk[k]) / dT
        q[k] = p1 + p2
        run = run + q[k]
        cdf[k] = run
        iw[k] = F32(nk[k] / (dT * q[k]))
    return cdf, iw, q, False


def three_tables(T, NB):
    """The tables the draw tests share: warm-up (uniform), skewed, and one with a zero-probability bucket (a table the
    rebuild never writes, t_mix > 0, but the draw must still respect: no sample lands in it)."""
    out = {"warmup": uniform_table(T, NB)}
    _, e = edges(T, NB)
    nk = np.diff(e).astype(F64)
    for name, zero in (("skewed", False), ("zero_bucket", True)):
        p = (np.arange(NB, dtype=F64) + 1.0) ** 2
        if zero and NB > 1:
            p[NB // 2] = 0.0
        q = p / p.sum()
        cdf = np.cumsum(q)
        with np.errstate(divide="ignore"):
            iw = np.where(q > 0, nk / (F64(T) * np.where(q > 0, q, 1.0)), 0.0).astype(F32)
        out[name] = (cdf, iw)
    return out
