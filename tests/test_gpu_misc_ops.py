"""Direct tests of the small-op kernels of csrc/misc.hip (EmbedFC, the MSE loss and its accumulating form, the forward
perturbation, the C_in = 1 / C_out = 1 3x3 convolutions, the transposes) and of cdm_gemm_x16 against plain fp64
references on the CPU (GPU box only).  The references are tests/_misc_ref.py; tests/test_misc_refs_cpu.py holds them to
torch's fp64 operators and autograd.

Style of tests/test_gpu_norm_ops.py: derived bounds, buffers with sentinel-filled pads (777) that must stay untouched,
dyadic inputs that make fp32 arithmetic exact, rejection cases that must write nothing.

Tolerances (u = 2^-24; each test's docstring derives its count from the kernel):
  * a sequential fp32 chain of n multiply-adds: (n + 8) u sum|term|
  * an fp64 sum rounded once to fp32: 1 ulp(ref) + 2^-50 sum|term|
  * chunked fp32 reducers: n = ceil(pixels / P) + P, P = 256 / (C / 4) pixel lanes (norm-ops' chunked bound)
  * fp32 GELU': 4 u (1/2 + |erf|/2 + |x| pdf), the bound of test_gpu_norm_ops.py::test_avgpool_gelu
  * dyadic inputs: bit-equal / exact; the grids are chosen so that every partial sum stays below 2^24 units
    (asserted on the CPU by tests/test_misc_refs_cpu.py)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _misc_ref as M
from _misc_ref import SENT, U, check, exact, ulp, widen

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 8


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cdm_amd
    return cdm_amd.lib()


def _err():
    import cdm_amd
    return cdm_amd._lib.HipError


def _s():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype).to(DEV)


def Z(*shape, fill=SENT, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def G(n):
    """a flat output buffer of n values and a sentinel pad"""
    return Z(int(n) + PAD)


def Hh(t):
    _sync()
    return t.detach().cpu().numpy().astype(np.float64)


def take(t, *shape):
    """the first prod(shape) values of a G buffer; its pad must still hold the sentinel"""
    a = Hh(t).reshape(-1)
    n = int(np.prod(shape))
    assert a.size == n + PAD and (a[n:] == SENT).all(), "wrote past the end of its output"
    return a[:n].reshape(shape)


def untouched(*ts):
    return all(bool((Hh(t) == SENT).all()) for t in ts)


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def P(t, off=0):
    """device address of t (+ off elements); t stays alive until the test ends (launches are asynchronous)"""
    if t is None:
        return None
    _KEEP.append(t)
    return t.data_ptr() + off * t.element_size()


# ----------------------------------------------------------------------------------------------------------------
# transposes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("R,C", [(1, 1), (64, 64), (65, 63), (130, 7), (3, 200)])
def test_transposes(L, R, C, batch):
    """64 x 64 tiles through LDS: one tile, an exact tile, ragged tiles in both directions, several tiles"""
    a = np.arange(batch * R * C, dtype=np.float64).reshape(batch, R, C) - 17.0
    out = G(batch * R * C)
    L.cdm_transpose_batched(P(T(a)), batch, R, C, P(out), _s())
    exact(take(out, batch, C, R), a.transpose(0, 2, 1), "transpose_batched")
    if batch == 1:
        out1 = G(R * C)
        L.cdm_transpose(P(T(a)), R, C, P(out1), _s())
        exact(take(out1, C, R), a[0].T, "transpose")


# ----------------------------------------------------------------------------------------------------------------
# EmbedFC
# ----------------------------------------------------------------------------------------------------------------
def _mlp4(L, specs, seed):
    import cdm_amd
    rng = np.random.default_rng(seed)
    mlp = cdm_amd._lib.Mlp4()
    cases = []
    for k, (rows, in_dim, E) in enumerate(specs):
        d = M.embed_inputs(rng, rows, in_dim, E)
        dev = {n: T(v) for n, v in d.items()}
        w2t = G(E * E)
        L.cdm_transpose(P(dev["w2"]), E, E, P(w2t), _s())
        exact(take(w2t, E, E), d["w2"].T, f"w2t of slot {k}")
        sizes = dict(pre=rows * E, h=rows * E, out=rows * E, dpre=rows * E, dw1=E * in_dim, db1=E, dw2=E * E, db2=E)
        o = {n: G(sz) for n, sz in sizes.items()}
        m = mlp.m[k]
        m.x, m.rows, m.in_dim, m.E = P(dev["x"]), rows, in_dim, E
        m.w1, m.b1, m.w2, m.w2t, m.b2 = P(dev["w1"]), P(dev["b1"]), P(dev["w2"]), P(w2t), P(dev["b2"])
        m.dout = P(dev["dout"])
        for n in sizes:
            setattr(m, n, P(o[n]))
        cases.append((rows, in_dim, E, d, o))
    return mlp, cases                     # slots past the specs stay zeroed: rows = 0, E = 0


def _rel_l2(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("launch", ["A", "B"])
def test_embed_fwd_bwd(L, launch):
    """cdm_embed_fwd: fp64 evaluation rounded once.  pre and h within 1 ulp of the fp64 reference (the reference's own
    fp64 rounding can move a value across an fp32 rounding boundary, hence 1 ulp and not 1/2); out = b2 + sum_i w2t h
    with the unrounded h: 1 ulp + 2^-50 sum|term|.
    cdm_embed_bwd, stage by stage from the values the device stored: dpre = GELU'(pre) sum_j dout[j] w2[j][i] is a
    sequential fp32 chain of E fmas, one fp32 GELU' and one product: (E + 8) u sum_j|dout w2| |GELU'| + (the GELU'
    bound) |sum| + 1 ulp; dw2 / db2 (from dout, h) and dw1 / db1 (from the device's dpre, x) are fp64 sums rounded
    once.  Launch A: four MLPs of different E / rows (rows > 64: the dw2 kernel's chunk loop; E = 100: its edge
    guards; E = 8, 16: blocks past the tiles; E = 1024: the LDS limit); launch B: slot 0 only, the others zeroed.
    Then once end to end against torch fp64 autograd of Linear -> GELU -> Linear at the bars of test_gpu_blocks.py
    (1e-5 relative L2 forward, 1e-4 gradients): the stage references are wired like the real op."""
    mlp, cases = _mlp4(L, M.MLPS_A if launch == "A" else [M.MLP_B], 11)
    L.cdm_embed_fwd(ctypes.addressof(mlp), _s())
    L.cdm_embed_bwd(ctypes.addressof(mlp), _s())
    for k, (rows, in_dim, E, d, o) in enumerate(cases):
        what = f"launch {launch} slot {k} (rows {rows}, in {in_dim}, E {E})"
        pre, h, out, mag = M.embed_fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
        pre_d, h_d = take(o["pre"], rows, E), take(o["h"], rows, E)
        check(pre_d, pre, ulp(pre), what + " pre")
        check(h_d, h, ulp(h), what + " h")
        check(take(o["out"], rows, E), out, M.sum_bound(out, mag), what + " out")
        dpre_d = take(o["dpre"], rows, E)
        dpre, bound = M.embed_dpre(d["dout"], d["w2"], pre_d)
        check(dpre_d, dpre, bound, what + " dpre")
        g = M.embed_param_grads(d["dout"], h_d, dpre_d, d["x"])
        got = dict(dw2=take(o["dw2"], E, E), db2=take(o["db2"], E), dw1=take(o["dw1"], E, in_dim),
                   db1=take(o["db1"], E))
        for name, (ref, gmag) in g.items():
            check(got[name], ref, M.sum_bound(ref, gmag), f"{what} {name}")
        t = {n: torch.from_numpy(d[n]).requires_grad_() for n in ("x", "w1", "b1", "w2", "b2")}
        F = torch.nn.functional
        ot = F.linear(torch.nn.GELU()(F.linear(t["x"], t["w1"], t["b1"])), t["w2"], t["b2"])
        ot.backward(torch.from_numpy(d["dout"]))
        assert _rel_l2(take(o["out"], rows, E), ot.detach().numpy()) <= 1e-5, what
        for n, name in (("w1", "dw1"), ("b1", "db1"), ("w2", "dw2"), ("b2", "db2")):
            assert _rel_l2(got[name], t[n].grad.numpy()) <= 1e-4, f"{what} {name} end to end"


@pytest.mark.parametrize("in_dim", [1, 6])
def test_embed_input_grad(L, in_dim):
    """dx[b][k] = sum_i dpre_a w1_a + sum_i dpre_b w1_b: two sequential fp32 fma chains of Ea and Eb terms and one
    addition: (Ea + 8) u sum|a terms| + (Eb + 8) u sum|b terms| + 1 ulp"""
    rng = np.random.default_rng(in_dim)
    rows, Ea, Eb = 130, 16, 100
    da, wa = M.gauss(rng, (rows, Ea)), M.gauss(rng, (Ea, in_dim))
    db, wb = M.gauss(rng, (rows, Eb)), M.gauss(rng, (Eb, in_dim))
    dx = G(rows * in_dim)
    L.cdm_embed_input_grad(P(T(da)), P(T(wa)), Ea, P(T(db)), P(T(wb)), Eb, rows, in_dim, P(dx), _s())
    ref, bound = M.embed_input_grad(da, wa, db, wb)
    check(take(dx, rows, in_dim), ref, bound, "input_grad, two inputs")
    dx1 = G(rows * in_dim)
    L.cdm_embed_input_grad(P(T(da)), P(T(wa)), Ea, None, None, 0, rows, in_dim, P(dx1), _s())
    ref, bound = M.embed_input_grad(da, wa)
    check(take(dx1, rows, in_dim), ref, bound, "input_grad, one input")
    # against autograd of dpre . w1 (the wiring: w1 is [E][in_dim], not its transpose)
    xt = torch.zeros(rows, in_dim, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.linear(xt, torch.from_numpy(wa)) * torch.from_numpy(da)).sum().backward()
    assert _rel_l2(take(dx1, rows, in_dim), xt.grad.numpy()) <= 1e-4


def test_embed_rejects(L):
    """E = 1025 in any slot is refused by both entry points; cdm_embed_input_grad refuses in_dim = 0 and negative rows
    and returns 0 for rows = 0: nothing is launched, every output keeps its sentinel"""
    E = _err()
    for slot in range(4):
        mlp, cases = _mlp4(L, [M.MLP_B], 3)
        mlp.m[slot].E = 1025
        with pytest.raises(E):
            L.cdm_embed_fwd(ctypes.addressof(mlp), _s())
        with pytest.raises(E):
            L.cdm_embed_bwd(ctypes.addressof(mlp), _s())
        assert untouched(*cases[0][4].values())
    a = T(np.ones((4, 8))); dx = G(32)
    for rows, in_dim in [(4, 0), (-1, 2)]:
        with pytest.raises(E):
            L.cdm_embed_input_grad(P(a), P(a), 4, None, None, 0, rows, in_dim, P(dx), _s())
    assert L.cdm_embed_input_grad(P(a), P(a), 4, None, None, 0, 0, 2, P(dx), _s()) == 0
    assert untouched(dx)


# ----------------------------------------------------------------------------------------------------------------
# cdm_mse
# ----------------------------------------------------------------------------------------------------------------
def _run_mse(L, pred, noise, gn, nb, loss=True, dbias=True, counter=5):
    n = pred.size
    dpred, partial = G(n), G(2 * nb)
    lo = G(1) if loss else None
    db = G(1) if dbias else None
    cnt = T(np.array([counter, -9]), torch.int32) if counter is not None else None
    L.cdm_mse(P(T(pred)), P(T(noise)), n, float(gn), P(dpred), P(partial), nb, P(lo), P(db), P(cnt), _s())
    _sync()
    return dpred, partial, lo, db, cnt


@pytest.mark.parametrize("nb", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_mse(L, n, nb):
    """Dyadic pred / noise (multiples of 2^-3 in [-1, 1]): d, d^2 and every partial sum of d^2 are exact for n <= 65536
    (tests/test_misc_refs_cpu.py).  All 2 nb partials are rewritten, with the block's own sums; an idle block's are 0.
    grad_numel a power of two: the scale is one, dpred = d scale and dbias = sum dpred are exact; loss = float(sum d^2
    (1 / n)) in fp64: within 1 ulp of the exact mean, exact where n is a power of two.
    grad_numel = 1.5 n (ragged data parallel: the gradient's divisor is not this rank's n): dpred is bit-equal to the
    fp32 product (pred - noise) * float(2 / grad_numel); dbias = sum dpred is then a sum of rounded values.  Its fold:
    a thread adds ceil(n / (256 nb)) terms in sequence, the wave butterfly adds 6 levels, the 4 wave sums are added
    (4), the finalize adds the nb block partials in fp64 and rounds once (counted as nb additions), and the
    vocabulary's + 8: (ceil(n / (256 nb)) + 6 + 4 + nb + 8) u sum|g|."""
    rng = np.random.default_rng(n * 100 + nb)
    pred, noise = M.mse_inputs(rng, n)
    d = pred - noise
    idle = np.arange(nb) * 256 >= n
    for gn in (4096.0, 1.5 * n):
        dpred, partial, lo, db, cnt = _run_mse(L, pred, noise, gn, nb)
        what = f"mse n={n} nb={nb} grad_numel={gn}"
        g = (d.astype(np.float32) * np.float32(2.0 / gn)).astype(np.float64)
        exact(take(dpred, n), g, what + " dpred")
        part = take(partial, nb, 2)
        exact(part[:, 0], M.mse_block_sums(d * d, n, nb), what + " partial sum d^2")
        assert (part[idle] == 0).all(), what + ": an idle block's partials are not zero"
        loss_ref = (d * d).sum() / n
        check(take(lo, 1), [loss_ref], ulp(loss_ref), what + " loss")
        if n & (n - 1) == 0:
            exact(take(lo, 1), [loss_ref], what + " loss (n a power of two)")
        if gn == 4096.0:
            assert np.array_equal(g, d * 2.0 / gn)
            exact(part[:, 1], M.mse_block_sums(g, n, nb), what + " partial sum dpred")
            exact(take(db, 1), [g.sum()], what + " dbias")
        else:
            k = M.mse_dbias_k(n, nb)
            check(part[:, 1], M.mse_block_sums(g, n, nb), k * U * M.mse_block_sums(np.abs(g), n, nb),
                  what + " partial sum dpred")
            check(take(db, 1), [g.sum()], k * U * np.abs(g).sum(), what + " dbias")
        assert cnt.cpu().tolist() == [5, -9], what + ": the non-finite counter moved on finite data"


def test_mse_counter_and_optional_outputs(L):
    rng = np.random.default_rng(1)
    n, nb = 257, 3
    pred, noise = M.mse_inputs(rng, n)
    for bad in (np.inf, np.nan):
        p = pred.copy(); p[100] = bad
        _, _, lo, _, cnt = _run_mse(L, p, noise, 4096.0, nb)
        assert cnt.cpu().tolist() == [6, -9] and not np.isfinite(lo.cpu().numpy()[0])
    g = (pred - noise) * 2.0 / 4096.0
    for loss, dbias, counter in [(False, True, 5), (True, False, 5), (True, True, None), (False, False, None)]:
        dpred, partial, lo, db, cnt = _run_mse(L, pred, noise, 4096.0, nb, loss, dbias, counter)
        exact(take(dpred, n), g, "dpred with null outputs")
        if lo is not None:
            exact(take(lo, 1), [f32_1((pred - noise) ** 2, n)], "loss with null outputs")
        if db is not None:
            exact(take(db, 1), [g.sum()], "dbias with null outputs")
    E = _err()
    for gn in (0.0, -1.0, float("nan")):
        dpred, partial, lo, db = G(n), G(2 * nb), G(1), G(1)
        with pytest.raises(E):
            L.cdm_mse(P(T(pred)), P(T(noise)), n, gn, P(dpred), P(partial), nb, P(lo), P(db), None, _s())
        assert untouched(dpred, partial, lo, db)


def f32_1(sq, n):
    """float(sum (1 / n)) as the finalize computes it (fp64 product, one rounding)"""
    return float(np.float32(sq.sum() * (1.0 / n)))


# ----------------------------------------------------------------------------------------------------------------
# cdm_mse_accum, cdm_perturb
# ----------------------------------------------------------------------------------------------------------------
N3, T7 = 3, 7
T_PER = np.array([1, 7, 4])


def _tables(rng):
    """mul / div of powers of two, indexed by the step 0..T"""
    return 2.0 ** rng.integers(-2, 3, size=T7 + 1), 2.0 ** rng.integers(-2, 3, size=T7 + 1)


def _accum(L, pred, noise, nstride, HW, t, cur_i, mul, div, acc0):
    acc = G(N3)
    acc[:N3] = T(acc0)
    L.cdm_mse_accum(P(T(pred)), P(T(noise)), nstride, T7, N3, HW, P(T(t, torch.int32)) if t is not None else None,
                    P(T(np.array([cur_i]), torch.int32)) if cur_i is not None else None, P(T(mul)), P(T(div)), P(acc),
                    _s())
    return take(acc, N3)


@pytest.mark.parametrize("HW", [1, 100, 256, 257, 1000])
def test_mse_accum(L, HW):
    """acc[n] += (mean_p (pred - noise)^2 * mul[i]) / div[i].  Dyadic data: sum d^2 is exact (at most 1000 x 256 units of
    2^-6), so the result is the four correctly rounded fp32 operations / HW, * mul, / div, += of _misc_ref.mse_accum32
    bit for bit (mul and div powers of two; acc starts from non-zero dyadic values since the kernel adds into it).
    Per-sample steps t = [1, 7, 4]; the cur_i form reads row T - i of a [T][N HW] noise table (every other row holds
    other data), or the one buffer with nstride = 0.
    Gaussian data: sum d^2 through a thread's chain of ceil(HW / 256) terms, 6 butterfly levels and 3 adds over the
    waves (+ 8, which covers each term's two roundings): k u term; then the three roundings of / HW, * mul, / div: 3 u
    term; then the accumulate: 1 ulp of the result."""
    rng = np.random.default_rng(HW)
    pred, noise = M.mse_inputs(rng, N3 * HW)
    mul, div = _tables(rng)
    acc0 = M.dyad(rng, N3) + 8.0
    got = _accum(L, pred, noise, 0, HW, T_PER, None, mul, div, acc0)
    exact(got, M.mse_accum32(acc0, pred, noise, HW, mul[T_PER], div[T_PER]), "mse_accum per-sample t")
    i = 3
    table = M.mse_inputs(rng, T7 * N3 * HW)[0].reshape(T7, N3 * HW)
    ref = M.mse_accum32(acc0, pred, table[T7 - i], HW, mul[[i] * N3], div[[i] * N3])
    if HW > 1:
        assert not np.array_equal(ref, M.mse_accum32(acc0, pred, table[T7 - i - 1], HW, mul[[i] * N3], div[[i] * N3]))
    exact(_accum(L, pred, table, N3 * HW, HW, None, i, mul, div, acc0), ref, "mse_accum cur_i, noise table")
    exact(_accum(L, pred, noise, 0, HW, None, i, mul, div, acc0),
          M.mse_accum32(acc0, pred, noise, HW, mul[[i] * N3], div[[i] * N3]), "mse_accum cur_i, nstride 0")
    # Gaussian
    pg, ng = M.gauss(rng, N3 * HW), M.gauss(rng, N3 * HW)
    mg, dg = M.f32(rng.random(T7 + 1) + 0.5), M.f32(rng.random(T7 + 1) + 0.5)
    a0 = M.gauss(rng, N3)
    term = ((pg - ng) ** 2).reshape(N3, HW).sum(axis=1) / HW * mg[T_PER] / dg[T_PER]
    check(_accum(L, pg, ng, 0, HW, T_PER, None, mg, dg, a0), a0 + term,
          (M.mse_accum_k(HW) + 3) * U * term + ulp(a0 + term), "mse_accum Gaussian")


def test_mse_accum_rejects(L):
    v = T(np.ones(N3 * 4)); acc = G(N3)
    with pytest.raises(_err()):
        L.cdm_mse_accum(P(v), P(v), 0, T7, N3, 4, None, None, P(v), P(v), P(acc), _s())
    assert untouched(acc)


@pytest.mark.parametrize("form", ["t", "cur_i", "cur_i_nstride0"])
def test_perturb(L, form):
    """out = sab[t] x + omab[t] nz and tin = float(t) / float(T) with separate fp32 roundings (the kernel switches
    contraction off): bit for bit against numpy fp32"""
    rng = np.random.default_rng(5)
    HW, i = 100, 3
    x, nz = M.gauss(rng, (N3, HW)), M.gauss(rng, (N3, HW))
    sab, omab = M.f32(rng.random(T7 + 1)), M.f32(rng.random(T7 + 1))
    table = M.gauss(rng, (T7, N3 * HW))
    if form == "t":
        steps, noise, nstride, src = T_PER, nz, 0, nz
        t_dev, c_dev = T(T_PER, torch.int32), None
    else:
        steps = np.array([i] * N3)
        noise, nstride, src = (table, N3 * HW, table[T7 - i].reshape(N3, HW)) if form == "cur_i" else (nz, 0, nz)
        t_dev, c_dev = None, T(np.array([i]), torch.int32)
    ref = M.perturb32(x, src, sab[steps], omab[steps])
    tin_ref = (steps.astype(np.float32) / np.float32(T7)).astype(np.float64)
    for with_tin in (True, False):
        out, tin = G(N3 * HW), G(N3)
        L.cdm_perturb(P(T(x)), P(T(noise)), P(t_dev), P(c_dev), nstride, P(T(sab)), P(T(omab)), N3, HW, T7, P(out),
                      P(tin) if with_tin else None, _s())
        exact(take(out, N3, HW), ref, f"perturb {form}")
        if with_tin:
            exact(take(tin, N3), tin_ref, f"perturb {form} tin")
        else:
            assert untouched(tin)
    out = G(N3 * HW)
    with pytest.raises(_err()):
        L.cdm_perturb(P(T(x)), P(T(nz)), None, None, 0, P(T(sab)), P(T(omab)), N3, HW, T7, P(out), None, _s())
    assert untouched(out)


# ----------------------------------------------------------------------------------------------------------------
# 3x3 convolutions, C_in = 1
# ----------------------------------------------------------------------------------------------------------------
WIDE = (1, 2, 2050, 4)       # wider than the row kernels' 2048 columns: the flat-pixel kernels serve it


def _gen(rng, shape, dyadic):
    return M.conv_dyad(rng, shape) if dyadic else M.gauss(rng, shape)


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES + [WIDE])
def test_conv_cin1_fwd(L, N, H, W, C, dyadic):
    """y[p][c] = b[c] + sum_tap x[p + tap] w9[tap][c] against torch's fp64 conv2d (tests/_misc_ref.py: the same
    sum tap by tap, held to conv2d on the CPU): a chain of 9 fmas from the bias, 11 u (|b| + sum|x w|); dyadic data
    (multiples of 2^-4 in [-2, 2]: 9 x 1024 + 512 units of 2^-8) bit-equal.  ldy = C + 4: the pad columns keep the
    sentinel.  amax is a running max: max(prefill, max|stored y|) exactly."""
    rng = np.random.default_rng(H * W + C + dyadic)
    x, w9, b = _gen(rng, (N, H, W), dyadic), _gen(rng, (9, C), dyadic), _gen(rng, C, dyadic)
    ld = C + 4
    for relu in (0, 1):
        ref, mag = M.cin1_fwd(x, w9, b, relu)
        for seed in (0.0, 1000.0):
            y = Z(N, H, W, ld); am = T(np.array([seed]))
            L.cdm_conv3x3_cin1_fwd(P(T(x)), N, H, W, P(T(w9)), P(T(b)), P(y), ld, C, relu, P(am), _s())
            o = Hh(y)
            assert (o[..., C:] == SENT).all(), "wrote outside its channel slice"
            check(o[..., :C], ref, 0.0 if dyadic else 11 * U * mag, f"cin1_fwd relu={relu}")
            assert float(Hh(am)[0]) == max(seed, float(np.abs(o[..., :C]).max()))
            assert float(np.abs(ref).max()) < 1000.0
    y = Z(N, H, W, ld)
    L.cdm_conv3x3_cin1_fwd(P(T(x)), N, H, W, P(T(w9)), P(T(b)), P(y), ld, C, 0, None, _s())      # amax == NULL
    check(Hh(y)[..., :C], M.cin1_fwd(x, w9, b, 0)[0], 0.0 if dyadic else 11 * U * mag, "cin1_fwd no amax")


@pytest.mark.parametrize("C", [6, 1028])
def test_conv_cin1_rejects(L, C):
    N, H, W = 1, 2, 2
    Ca = C + 6
    x = T(np.ones((N, H, W))); v = T(np.ones((10, Ca))); y = Z(N, H, W, Ca); slab = Z(N, 10, Ca)
    E = _err()
    with pytest.raises(E):
        L.cdm_conv3x3_cin1_fwd(P(x), N, H, W, P(v), P(v), P(y), Ca, C, 0, None, _s())
    with pytest.raises(E):
        L.cdm_conv3x3_cin1_wgrad(P(y), Ca, P(x), N, H, W, C, 128, P(slab), _s())
    assert untouched(y, slab)


def _check_slab(got, terms, csize, C, dyadic, what):
    """every partial [n][chunk][r][c] against the fp64 sum over that chunk's own pixels"""
    ref = M.chunk_sums(terms, csize)
    px = min(csize, terms.shape[1])
    bound = 0.0 if dyadic else M.chain_bound(M.lanes_n(C, px), M.chunk_sums(np.abs(terms), csize))
    check(got, ref, bound, what)


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES)
def test_conv_cin1_wgrad(L, N, H, W, C, dyadic):
    """partials [n][chunk][10][C]: rows 0..8 sum_p dy[p][c] x[p + tap], row 9 sum_p dy[p][c] over the chunk's pixels.
    A lane adds its ceil(csize / P) pixels in sequence (P = 256 / (C / 4) lanes), the fold adds the P lanes:
    (ceil(csize / P) + P + 8) u sum|term| (norm-ops' chunked bound); dyadic data exact (at most 900 x 1024 units)."""
    rng = np.random.default_rng(H * W + C + 2 * dyadic)
    dy, x = _gen(rng, (N, H, W, C), dyadic), _gen(rng, (N, H, W), dyadic)
    terms = M.cin1_wgrad_terms(dy, x)
    HW, ld = H * W, C + 4
    dyd, xd = T(widen(dy, ld, 0)), T(x)
    for csize in (128, 50, HW + 5):
        nch = -(-HW // csize)
        slab = G(N * nch * 10 * C)
        L.cdm_conv3x3_cin1_wgrad(P(dyd), ld, P(xd), N, H, W, C, csize, P(slab), _s())
        _check_slab(take(slab, N, nch, 10, C), terms, csize, C, dyadic, f"cin1_wgrad csize={csize}")


# ----------------------------------------------------------------------------------------------------------------
# 3x3 convolutions, C_out = 1
# ----------------------------------------------------------------------------------------------------------------
BAND_EXTRA = [(2, 4, 128, 16), (1, 2, 256, 32)]      # 512- and 768-pixel halo images of the band kernel


def band_ok(H, W, C, ld):
    """the launcher's conditions for the band form of the C_out = 1 forward"""
    return C % 16 == 0 and W <= 256 and 256 % W == 0 and H % (256 // W) == 0 and ld % 4 == 0


def test_band_conditions_cover_both_forms():
    took = [band_ok(H, W, C, C + 4) for _, H, W, C in M.CONV_SHAPES + BAND_EXTRA]
    assert sum(took) >= 3 and len(took) - sum(took) >= 2


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES + BAND_EXTRA)
def test_conv_cout1_fwd(L, N, H, W, C, dyadic):
    """out[p] = b + sum_{tap, c} z[p + tap][c] w[c][tap] against torch's fp64 conv2d.  Flat form: a lane's chain of 36
    fmas, then the fold of C / 4 lanes and the bias; band form: a chain of C fmas per tap, then 9 adds.  Both are
    within (9 C + C / 4 + 8) u (|b| + sum|z w|), the count of every multiply-add and fold step.  Shapes the band form
    takes (W | 256, (256 / W) | H, C % 16 == 0) and shapes it does not: there the flat kernel serves the call and
    cdm_conv3x3_cout1_fwd_gn refuses.  _gn: the input is relu(y gs + gt) per (sample, channel); y, gs, gt dyadic, so
    the gate equals the reference's element for element."""
    rng = np.random.default_rng(H * W + C + 3 * dyadic)
    z, w = _gen(rng, (N, H, W, C), dyadic), _gen(rng, (C, 9), dyadic)
    b = 0.375
    ld = C + 4
    zd, wd, bd = T(widen(z, ld, 0)), T(w), T(np.array([b]))
    k = (9 * C + C // 4 + 8) * U
    out = G(N * H * W)
    L.cdm_conv3x3_cout1_fwd(P(zd), ld, N, H, W, C, P(wd), P(bd), P(out), _s())
    ref, mag = M.cout1_fwd(z, w, b)
    tref = M.torch_cout1(z, w, b)[0].detach().numpy()
    check(ref, tref, 2.0 ** -40 * mag, "reference against conv2d")
    check(take(out, N, H, W), tref, k * mag, "cout1_fwd")
    y = M.conv_dyad(rng, (N, H, W, C)); gs = M.conv_dyad(rng, (N, C)); gt = M.conv_dyad(rng, (N, C))
    yd, gsd, gtd = T(widen(y, ld, 0)), T(gs), T(gt)
    og = G(N * H * W)
    if band_ok(H, W, C, ld):
        L.cdm_conv3x3_cout1_fwd_gn(P(yd), ld, N, H, W, C, P(gsd), P(gtd), P(wd), P(bd), P(og), _s())
        ref, mag = M.cout1_fwd(y, w, b, gs, gt)
        check(take(og, N, H, W), ref, k * mag, "cout1_fwd_gn")
    else:
        with pytest.raises(_err()):
            L.cdm_conv3x3_cout1_fwd_gn(P(yd), ld, N, H, W, C, P(gsd), P(gtd), P(wd), P(bd), P(og), _s())
        assert untouched(og)


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES + [WIDE])
def test_conv_cout1_dgrad(L, N, H, W, C, dyadic):
    """dz[p][c] = sum_tap deps[p - tap] w[c][tap] against torch fp64 autograd of conv2d: a chain of 9 fmas,
    11 u sum|deps w|; dyadic data exact.  lddz = C + 4."""
    rng = np.random.default_rng(H * W + C + 5 * dyadic)
    deps, w = _gen(rng, (N, H, W), dyadic), _gen(rng, (C, 9), dyadic)
    ld = C + 4
    dz = Z(N, H, W, ld)
    L.cdm_conv3x3_cout1_dgrad(P(T(deps)), N, H, W, C, P(T(w)), P(dz), ld, _s())
    ref, mag = M.cout1_dgrad(deps, w)
    _, zt, _ = M.torch_cout1(np.zeros((N, H, W, C)), w, 0.0)
    torch.nn.functional.conv2d(zt, torch.from_numpy(w.reshape(1, C, 3, 3)), padding=1)[:, 0].backward(
        torch.from_numpy(deps))
    tref = zt.grad.numpy().transpose(0, 2, 3, 1)
    check(ref, tref, 2.0 ** -40 * mag, "reference against autograd")
    o = Hh(dz)
    assert (o[..., C:] == SENT).all(), "wrote outside its channel slice"
    check(o[..., :C], tref, 0.0 if dyadic else 11 * U * mag, "cout1_dgrad")


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES)
def test_conv_cout1_wgrad(L, N, H, W, C, dyadic):
    """Chunk form: partial [n][chunk][9][C] = sum_{p in chunk} deps[p] z[p + tap][c].  Band form (csize = -R): a block
    owns R whole rows of z and takes deps from the halo, so partial [band][9][C] = sum_{q in band} z[q][c] deps[q -
    tap]: the same total, split differently.  Either is a lane's sequential chain over its share of the pixels and the
    fold over the P = 256 / (C / 4) lanes: (ceil(pixels / P) + P + 8) u sum|term|; dyadic data exact.  The totals
    over the partials equal conv2d's weight gradient (torch fp64 autograd).  cdm_conv3x3_cout1_wgrad_gn with gs / gt
    null is the plain band form bit for bit; with them z = relu(y gs + gt) (dyadic: the gate matches)."""
    rng = np.random.default_rng(H * W + C + 7 * dyadic)
    deps, z = _gen(rng, (N, H, W), dyadic), _gen(rng, (N, H, W, C), dyadic)
    HW, ld = H * W, C + 4
    dd, zd = T(deps), T(widen(z, ld, 0))
    out, _, wt = M.torch_cout1(z, np.zeros((C, 9)), 0.0)
    out.backward(torch.from_numpy(deps))
    dw = wt.grad.numpy().reshape(C, 9).T                                       # [9][C]
    ct = M.cout1_wgrad_chunk_terms(deps, z)
    for csize in (128, 50):
        nch = -(-HW // csize)
        slab = G(N * nch * 9 * C)
        L.cdm_conv3x3_cout1_wgrad(P(dd), P(zd), ld, N, H, W, C, csize, P(slab), _s())
        got = take(slab, N, nch, 9, C)
        _check_slab(got, ct, csize, C, dyadic, f"cout1_wgrad csize={csize}")
        tb = M.chain_bound(M.lanes_n(C, min(csize, HW)), np.abs(ct).sum(axis=(0, 1)))
        check(got.sum(axis=(0, 1)), dw, 0.0 if dyadic else tb, f"cout1_wgrad csize={csize} total")
    bt = M.cout1_wgrad_band_terms(deps, z)
    y = M.conv_dyad(rng, (N, H, W, C)); gs = M.conv_dyad(rng, (N, C)); gt = M.conv_dyad(rng, (N, C))
    yd, gsd, gtd = T(widen(y, ld, 0)), T(gs), T(gt)
    gnt = M.cout1_wgrad_band_terms(deps, y, gs, gt)
    for R in sorted({1, 2, H}):
        nbands = N * (H // R)
        slab = G(nbands * 9 * C)
        if H % R:
            with pytest.raises(_err()):
                L.cdm_conv3x3_cout1_wgrad(P(dd), P(zd), ld, N, H, W, C, -R, P(slab), _s())
            assert untouched(slab)
            continue
        L.cdm_conv3x3_cout1_wgrad(P(dd), P(zd), ld, N, H, W, C, -R, P(slab), _s())
        got = take(slab, nbands, 9, C)
        k = M.lanes_n(C, R * W)
        check(got, M.band_sums(bt, W, R), 0.0 if dyadic else M.chain_bound(k, M.band_sums(np.abs(bt), W, R)),
              f"cout1_wgrad band R={R}")
        check(got.sum(axis=0), dw, 0.0 if dyadic else M.chain_bound(k, np.abs(bt).sum(axis=(0, 1))),
              f"cout1_wgrad band R={R} total")
        slab2 = G(nbands * 9 * C)
        L.cdm_conv3x3_cout1_wgrad_gn(P(dd), P(zd), ld, N, H, W, C, None, None, -R, P(slab2), _s())
        _sync()
        assert torch.equal(slab2, slab), "wgrad_gn with gs / gt null differs from the band form"
        slab3 = G(nbands * 9 * C)
        L.cdm_conv3x3_cout1_wgrad_gn(P(dd), P(yd), ld, N, H, W, C, P(gsd), P(gtd), -R, P(slab3), _s())
        check(take(slab3, nbands, 9, C), M.band_sums(gnt, W, R),
              M.chain_bound(k, M.band_sums(np.abs(gnt), W, R)), f"cout1_wgrad_gn R={R}")


def test_conv_cout1_rejects(L):
    """H % R != 0, csize >= 0 to _gn, gs without gt, a leading dimension that is no multiple of 4, a band whose deps
    image and fold exceed 64 KiB of LDS (66 x 130 floats + 36 KiB), C % 4 and C > 1024"""
    E = _err()
    N, H, W, C = 1, 64, 128, 4
    deps = T(np.ones((N, H, W))); z = T(np.ones((N, H, W, C + 4))); v = T(np.ones((N, 1032))); slab = G(N * H * 9 * C)
    w = T(np.ones((1032, 9))); out = G(N * H * W); dz = Z(N, H, W, C + 4)
    gn = L.cdm_conv3x3_cout1_wgrad_gn
    for args in [(C, P(v), P(v), -5, C + 4),            # H % R
                 (C, P(v), P(v), 0, C + 4), (C, None, None, 128, C + 4),     # csize >= 0
                 (C, P(v), None, -1, C + 4),            # gs without gt
                 (C, None, None, -1, C + 2),            # ldy % 4
                 (C, None, None, -64, C + 4),           # LDS
                 (6, None, None, -1, C + 4), (1028, None, None, -1, C + 4)]:
        Cc, gs, gt, csize, ld = args
        with pytest.raises(E):
            gn(P(deps), P(z), ld, N, H, W, Cc, gs, gt, csize, P(slab), _s())
    with pytest.raises(E):
        L.cdm_conv3x3_cout1_wgrad(P(deps), P(z), C + 4, N, H, W, C, -64, P(slab), _s())
    for Cc in (6, 1028):
        with pytest.raises(E):
            L.cdm_conv3x3_cout1_wgrad(P(deps), P(z), C + 4, N, H, W, Cc, 128, P(slab), _s())
        with pytest.raises(E):
            L.cdm_conv3x3_cout1_fwd(P(z), C + 4, N, H, W, Cc, P(w), P(v), P(out), _s())
        with pytest.raises(E):
            L.cdm_conv3x3_cout1_dgrad(P(deps), N, H, W, Cc, P(w), P(dz), C + 4, _s())
    # _gn: a null gs, a leading dimension that is no multiple of 4 (a shape the band form would take)
    zb = T(np.ones((1, 16, 16, 20)))
    for gs, gt, ld in [(None, P(v), 20), (P(v), None, 20), (P(v), P(v), 18)]:
        with pytest.raises(E):
            L.cdm_conv3x3_cout1_fwd_gn(P(zb), ld, 1, 16, 16, 16, gs, gt, P(w), P(v), P(out), _s())
    assert untouched(slab, out, dz)


# ----------------------------------------------------------------------------------------------------------------
# cdm_gemm_x16
# ----------------------------------------------------------------------------------------------------------------
def _wx(L, w, K, N, nterm):
    """the split image of B [K][N] and its max (h3) as tests/test_gpu_kernels.py builds them (_split_h3 / _split)"""
    out = torch.empty(((K + 15) // 16) * 3 * N * 16, dtype=torch.bfloat16, device=DEV)
    if nterm == 4:
        am = torch.empty(1, device=DEV)
        L.cdm_amax_f32(P(w), K, N, N, P(am), 0, _s())
        L.cdm_split_f16x2(P(w), N, K, N, P(am), P(out), _s())
        return out, am
    L.cdm_split_bf16x3(P(w), N, K, N, P(out), _s())
    return out, None


@pytest.mark.parametrize("nterm", [4, 1])
@pytest.mark.parametrize("K,N", [(36, 132), (256, 4096)])
@pytest.mark.parametrize("M_", [1, 5, 130])
def test_gemm_x16(L, M_, K, N, nterm):
    """C = A B + bias[n % bias_mod] on the 16-bit matrix cores, ldc = N + 4, amax_c a running max.
    nterm = 4 (scaled fp16 hi / lo, three products): fp32-class, held to the fp64 GEMM at the tolerance
    tests/test_gpu_kernels.py::test_conv3x3_h3_fp32_class applies to the h3 entry points (its _close: |err| <= 2e-5
    max|ref| + 1e-5).
    nterm = 1 (bf16 operands): the reference is the fp64 GEMM of the operands as the kernel rounds them, A and B to
    bf16 by round-to-nearest-even (built as test_bf16_halo_conv_vs_fp64 / tests/_bf16emu.py do, through torch's
    bfloat16 cast); the products of two bf16 values are exact in fp32, so only the fp32 accumulation of K terms and
    the bias remains: (K + 8) u (|bias| + sum|a b|)."""
    rng = np.random.default_rng(M_ + K + nterm)
    a, b = M.gauss(rng, (M_, K)), M.gauss(rng, (K, N), 0.05)
    ad, bd_ = T(a), T(b)
    wx, amw = _wx(L, bd_, K, N, nterm)
    ama = None
    if nterm == 4:
        ama = torch.empty(1, device=DEV)
        L.cdm_amax_f32(P(ad), M_, K, K, P(ama), 0, _s())
    if nterm == 1:
        bf = lambda v: torch.from_numpy(v).float().bfloat16().double().numpy()   # noqa: E731
        a, b = bf(a), bf(b)
    for bias_mod in (N, 32):
        bias = M.gauss(rng, bias_mod)
        bfull = bias[np.arange(N) % bias_mod]
        ref = a @ b + bfull
        mag = np.abs(a) @ np.abs(b) + np.abs(bfull)
        bound = (2e-5 * np.abs(ref).max() + 1e-5) if nterm == 4 else M.chain_bound(K, mag)
        for seed in (0.0, 1000.0):
            c = Z(M_, N + 4); am = T(np.array([seed]))
            L.cdm_gemm_x16(P(ad), K, M_, K, P(wx), P(ama), P(amw), N, P(c), N + 4, P(T(bias)), bias_mod, P(am), nterm,
                           _s())
            o = Hh(c)
            assert (o[:, N:] == SENT).all(), "wrote outside its columns"
            check(o[:, :N], ref, bound, f"gemm_x16 nterm={nterm} bias_mod={bias_mod}")
            assert float(Hh(am)[0]) == max(seed, float(np.abs(o[:, :N]).max()))
            assert float(np.abs(ref).max()) < 1000.0


def test_gemm_x16_rejects(L):
    """K % 4, N % 4, lda % 4, an nterm that is neither form, and the h3 form without its operand maxima"""
    E = _err()
    M_, K, N = 5, 36, 132
    a = T(np.ones((M_, K + 4))); w = T(np.ones((K + 4, N + 4)))
    wx, amw = _wx(L, w, K + 4, N + 4, 4)
    ama = T(np.array([1.0])); bias = T(np.ones(N + 4)); c = Z(M_, N + 8)
    for Kk, Nn, lda, nterm, x, y in [(K + 2, N, K + 4, 4, ama, amw), (K, N + 2, K + 4, 4, ama, amw),
                                     (K, N, K + 2, 4, ama, amw), (K, N, K + 4, 2, ama, amw),
                                     (K, N, K + 4, 4, None, amw), (K, N, K + 4, 4, ama, None)]:
        with pytest.raises(E):
            L.cdm_gemm_x16(P(a), lda, M_, Kk, P(wx), P(x), P(y), Nn, P(c), N + 8, P(bias), Nn, None, nterm, _s())
    assert untouched(c)
