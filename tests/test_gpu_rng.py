"""The device RNG against the host oracle tests/_rng_ref.py (GPU box only; tests/test_rng_refs_cpu.py holds the oracle to
the Random123 known answers and to a generator's statistics, so nothing statistical is needed here).

  * cdm_philox_uniform at (0, 1): bit-equal to the oracle over the tail n % 4 != 0, the grid-stride loop (the launch is
    capped at 8192 blocks of 256 threads of 4 elements), both key words, sub + *sub_dev mod 2^32, and the three streams
    whose named element is exactly 1.0f (u01's range is (0, 1]).
  * cdm_philox_uniform at (lo, hi): every element is lo + (hi - lo) u with two roundings or with one (an fma).
  * cdm_philox_randint: bit-equal.
  * cdm_philox_normal: per element within B = r (4 pi + 10) U + 2 U of the fp64 Box-Muller of the same fp32 uniforms.
  * every in-kernel normal draw (cdm_denoise, the DDIM forms, the blends, the jump) at numel = 1027: the stored value is
    the draw, and it is bit-equal to what cdm_philox_normal writes for the documented key and stream, which in turn is
    within B of the oracle; the neighbouring wrong key or stream gives other values.
  * cdm_flow_probe: equal to the oracle's uniforms compared with 0.5.
  * the argument checks of the three generators.

Every buffer has PAD sentinel values (777) past its end, which must be intact.  The 64-bit element index cannot be reached
in a test of a few seconds: the high counter word (q >> 32, e >> 34) is zero in every case here.
"""
import functools

import numpy as np
import pytest
import torch

import _rng_ref as R

pytestmark = pytest.mark.gpu

PAD, SENT = 8, 777
INVALID = 1                                    # hipErrorInvalidValue
N_BIG = 8192 * 256 * 4 + 5                     # one element quad past the block cap, and a tail
NS = [1, 3, 4, 5, 1023, 1024, 1025, N_BIG]
SEED_HL = 0x1234_5678_9ABC_DEF0
SEEDS = [0, 1, 0xFFFFFFFF, SEED_HL]
SUBS = [0, 3 << 24, 0xFFFFFFFF]
CTR = 7
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cdm_amd
    return cdm_amd.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _buf(n, dtype=torch.float32):
    return torch.full((int(n) + PAD,), SENT, dtype=dtype, device="cuda")


def _take(buf, n):
    """the n values of a padded buffer as numpy, after checking the pad"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[n:] == SENT).all(), "wrote past n"
    return h[:n]


def _ctr(v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def _uniform(L, n, lo, hi, seed, sub, ctr=None):
    out, c = _buf(n), _ctr(ctr)
    L.cdm_philox_uniform(_p(out), n, lo, hi, seed, sub, _p(c), _s())
    return _take(out, n)


def _normal(L, n, seed, sub, ctr=None):
    out, c = _buf(n), _ctr(ctr)
    L.cdm_philox_normal(_p(out), n, seed, sub, _p(c), _s())
    return _take(out, n)


def _randint(L, n, lo, hi, seed, sub, ctr=None):
    out, c = _buf(n, torch.int32), _ctr(ctr)
    L.cdm_philox_randint(_p(out), n, lo, hi, seed, sub, _p(c), _s())
    return _take(out, n)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"


@functools.lru_cache(maxsize=None)
def _ref_u01(n, seed, sub):
    return R.uniform_stream(n, 0.0, 1.0, seed, sub)[0]


@functools.lru_cache(maxsize=None)
def _ref_normal(n, seed, sub):
    return R.normal_stream64(n, seed, sub)


# ------------------------------------------------------------------------------------------------
# the generators
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_uniform01_bit_equal_over_sizes(L, n):
    """n around the 4-element quad and the 256-thread block, and N_BIG = 8192 * 256 * 4 + 5: the last quads are drawn
    by the second trip of the grid-stride loop."""
    got = _uniform(L, n, 0.0, 1.0, SEED_HL, 3 << 24)
    _same_bits(got, _ref_u01(n, SEED_HL, 3 << 24), f"n = {n}")
    assert got.min() > 0 and got.max() <= 1


def test_uniform01_bit_equal_over_keys_and_streams(L):
    """Both key words (seeds below and above 2^32), sub with and without the device counter; sub + *sub_dev wraps mod
    2^32.  Swapping the two halves of the seed is another stream."""
    n = 1025
    for seed in SEEDS:
        for sub in SUBS:
            _same_bits(_uniform(L, n, 0.0, 1.0, seed, sub), _ref_u01(n, seed, sub), f"seed {seed:#x} sub {sub:#x}")
            _same_bits(_uniform(L, n, 0.0, 1.0, seed, sub, CTR), _ref_u01(n, seed, (sub + CTR) & M32),
                       f"seed {seed:#x} sub {sub:#x} + counter")
    for seed in (SEED_HL, 1):
        swapped = ((seed << 32) | (seed >> 32)) & 0xFFFFFFFFFFFFFFFF
        a, b = _uniform(L, n, 0.0, 1.0, seed, 5), _uniform(L, n, 0.0, 1.0, swapped, 5)
        _same_bits(b, _ref_u01(n, swapped, 5), f"seed {swapped:#x}")
        assert not np.array_equal(a, b)


@pytest.mark.parametrize("seed,sub,word", [(0, 1543363, 0), (0, 674387, 1), (1234, 20278353, 3)])
def test_uniform01_reaches_one(L, seed, sub, word):
    """Words with v >> 8 == 0xFFFFFF (R.find_u_one; re-derived on the CPU by tests/test_rng_refs_cpu.py): the + 0.5f
    ties to even and the element is exactly 1.0f."""
    got = _uniform(L, word + 1, 0.0, 1.0, seed, sub)
    _same_bits(got, _ref_u01(word + 1, seed, sub))
    assert got[word] == np.float32(1.0)


@pytest.mark.parametrize("bound", [1.0, 1.0 / np.sqrt(2.0), 1.0 / np.sqrt(3.0)])
def test_uniform_affine_is_one_of_the_two_forms(L, bound):
    """(-bound, bound) for model.py's shortcut draw at 1, 2 and 3 input channels (and the trainer's (-1, 1)).  Each
    element equals lo + (hi - lo) u with the product and the sum rounded separately, or with one rounding (fma); every
    value lies in [lo, hi].
    At (-1, 1) the two forms are the same bits (hi - lo = 2: the product is exact), so the question does not arise for
    the trainer's draw or for single-channel maps.  At the other two bounds this build gives the one-rounding (fma)
    form on every element where the two differ (gfx950, ROCm 7.2, -O3: 2615 of 5124 elements at 1/sqrt(2) and 2694 at
    1/sqrt(3) differ between the forms, none of them unfused)."""
    lo, hi = np.float32(-bound), np.float32(bound)
    for n, seed, sub, ctr in ((1025, 0x5C0FFEE + 4242, 1, None), (4099, SEED_HL, 2 << 24, CTR)):
        got = _uniform(L, n, float(lo), float(hi), seed, sub, ctr)
        two, one = R.uniform_stream(n, lo, hi, seed, sub + (ctr or 0))
        is_two, is_one = _bits(got) == _bits(two), _bits(got) == _bits(one)
        differ = _bits(two) != _bits(one)
        print(f"bound {bound:.6f} n {n}: forms differ on {differ.sum()}, device == two-rounding on "
              f"{(is_two & differ).sum()}, == one-rounding on {(is_one & differ).sum()}")
        assert (is_two | is_one).all(), f"{(~(is_two | is_one)).sum()} elements are neither form"
        assert got.min() >= lo and got.max() <= hi
        if bound == 1.0:
            assert not differ.any()
        else:
            assert differ.any()


@pytest.mark.parametrize("lo,hi", [(1, 1500), (0, 0), (-5, 5), (1, 2 ** 31 - 1)])
def test_randint_bit_equal(L, lo, hi):
    for n in (1, 255, 256, 257):
        for seed, sub, ctr in ((SEED_HL, 1 << 24, None), (1, 0xFFFFFFFF, CTR)):
            got = _randint(L, n, lo, hi, seed, sub, ctr)
            want = R.randint_stream(n, lo, hi, seed, (sub + (ctr or 0)) & M32)
            assert got.dtype == np.int32 and np.array_equal(got, want), (n, seed, sub, ctr)
            assert got.min() >= lo and got.max() <= hi


def _normal_ratio(got, n, seed, sub):
    z64, r = _ref_normal(n, seed, sub)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    return float((np.abs(got.astype(np.float64) - z64) / R.normal_bound(r)).max())


@pytest.mark.parametrize("n", NS)
def test_normal_within_bound_over_sizes(L, n):
    """|z - z64| <= B = r (4 pi + 10) U + 2 U per element, U = 2^-24, r = sqrt(-2 ln u1) from the oracle: r 4 pi U for
    the two roundings of an angle up to 2 pi, 4 U r for a two-ulp sincosf at magnitude 1, the rest a one-ulp logf, a
    one-ulp sqrtf and the final product.  z64 is fp64 Box-Muller of the same fp32 u1, u2, so a wrong word, pair, element
    order, key or counter is an error of order 1, not of order U.
    Measured on an MI355X (ROCm 7.2): the largest |z - z64| / B is 0.304, at N_BIG (0.276 at n = 1025, 0.293 over the
    keys and streams of the next test)."""
    ratio = _normal_ratio(_normal(L, n, SEED_HL, 3 << 24), n, SEED_HL, 3 << 24)
    print(f"normal n = {n}: max |z - z64| / B = {ratio:.3f}")
    assert ratio <= 1.0


def test_normal_within_bound_over_keys_and_streams(L):
    n, worst = 1025, 0.0
    for seed in SEEDS:
        for sub in SUBS:
            worst = max(worst, _normal_ratio(_normal(L, n, seed, sub), n, seed, sub),
                        _normal_ratio(_normal(L, n, seed, sub, CTR), n, seed, (sub + CTR) & M32))
    print(f"normal over keys and streams: max |z - z64| / B = {worst:.3f}")
    assert worst <= 1.0
    swapped = ((SEED_HL << 32) | (SEED_HL >> 32)) & 0xFFFFFFFFFFFFFFFF
    a, b = _normal(L, n, SEED_HL, 5), _normal(L, n, swapped, 5)
    assert _normal_ratio(b, n, swapped, 5) <= 1.0 and not np.array_equal(a, b)
    # the normal and the uniform domain words: other words for one (key, counter)
    assert not np.array_equal(R._quad_words(n, SEED_HL, 5, R.NORMAL_C3), R._quad_words(n, SEED_HL, 5, R.UNIFORM_C3))


# ------------------------------------------------------------------------------------------------
# the in-kernel draws
# ------------------------------------------------------------------------------------------------
NUMEL = 1027                      # not a multiple of 4, more than one block of 256 threads and more than one of 1024
SEED, SEED_DEV = 1234, 99
KEY = SEED ^ SEED_DEV
TT = 12                           # the tables' length - 1 (timesteps, or positions)


class _Draws:
    """Inputs that make each kernel store its draw: zeros for x / eps / known, ones for the mask and for the coefficient
    of the draw, zeros for every other coefficient.  The stored value is 0 + 1 * z, so only the sign of a zero can differ
    from z."""

    def __init__(self, L):
        self.L = L
        self.zero = torch.zeros(NUMEL, device="cuda")
        self.ones = torch.ones(NUMEL, device="cuda")
        self.t0 = torch.zeros(TT + 1, device="cuda")
        self.t1 = torch.ones(TT + 1, device="cuda")
        self.zseed = torch.tensor([SEED_DEV], dtype=torch.int64, device="cuda")

    def gen(self, key, sub):
        """cdm_philox_normal's stream under (key, sub), itself held to the oracle"""
        got = _normal(self.L, NUMEL, key, sub)
        assert _normal_ratio(got, NUMEL, key, sub) <= 1.0
        return got

    def out(self):
        return torch.full((NUMEL + PAD,), float(SENT), device="cuda")


@pytest.fixture(scope="module")
def D(L):
    return _Draws(L)


def _is_draw(got, want, what):
    """bit-equal but for the sign of a zero (0 + 1 * (-0) is +0)"""
    both_zero = (got == 0) & (want == 0)
    bad = np.nonzero((_bits(got) != _bits(want)) & ~both_zero)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"


def test_denoise_draws_key_and_timestep(L, D):
    """cdm_denoise at i = 5: x = eps = 0, coef = 0, sa = sb = 1 stores z = Philox(seed ^ *seed_dev, stream i).  At i = 1
    it draws nothing and stores the mean, 0."""
    def run(i, seed_dev=D.zseed):
        out, cur_i = D.out(), _ctr(i)
        L.cdm_denoise(_p(D.zero), _p(out), None, NUMEL, _p(D.zero), 0, 0.0, _p(cur_i), _p(D.t0), _p(D.t1), _p(D.t1),
                      None, NUMEL, SEED, _p(seed_dev), None, None, TT, _s())
        return _take(out, NUMEL)
    _is_draw(run(5), D.gen(KEY, 5), "cdm_denoise")
    _is_draw(run(5, None), D.gen(SEED, 5), "cdm_denoise without seed_dev")
    assert not run(1).any()


def test_ddim_step_draws_key_and_timestep(L, D):
    """cdm_ddim_step at position k = 3 of the timestep i = 9: stream i under the plain run key, not stream k."""
    k, i = 3, 9
    out, cur_i, cur_k = D.out(), _ctr(i), _ctr(k)
    L.cdm_ddim_step(_p(D.zero), _p(out), None, NUMEL, _p(D.zero), 0, 0.0, _p(cur_i), _p(cur_k), _p(D.t0), _p(D.t0),
                    _p(D.t1), TT, None, NUMEL, SEED, _p(D.zseed), None, None, _s())
    got = _take(out, NUMEL)
    _is_draw(got, D.gen(KEY, i), "cdm_ddim_step")
    assert not np.array_equal(got, D.gen(KEY, k)), "keyed by the position"


@pytest.mark.parametrize("guided", [False, True], ids=["pos", "guided"])
def test_ddim_step_pos_draws_domain_and_position(L, D, guided):
    """cdm_ddim_step_pos and cdm_ddim_step_guided (zeta = 0) at k = 3: stream k under key ^ STEP_NOISE_DOMAIN, not under
    the plain key."""
    k = 3
    out, cur_k = D.out(), _ctr(k)
    args = (_p(D.zero), _p(out), None, NUMEL, _p(D.zero), 0, 0.0, _p(cur_k), _p(D.t0), _p(D.t0), _p(D.t1), TT, None,
            NUMEL, SEED, _p(D.zseed), None, None)
    if guided:
        L.cdm_ddim_step_guided(*args, None, None, None, 0.0, 1, _s())
    else:
        L.cdm_ddim_step_pos(*args, _s())
    got = _take(out, NUMEL)
    _is_draw(got, D.gen(KEY ^ R.STEP_NOISE_DOMAIN, k), "position-keyed z")
    assert not np.array_equal(got, D.gen(KEY, k)), "the plain key"


@pytest.mark.parametrize("form", ["ancestral", "strided"])
@pytest.mark.parametrize("fresh", [1, 0])
def test_mask_blend_xi_draws_domain_and_level(L, D, form, fresh):
    """cdm_mask_blend with known = 0, sab = 0, somab = 1, mask = 1 stores xi = Philox(key ^ KNOWN_NOISE_DOMAIN, stream
    fresh ? j : 0); j = i - 1 in the ancestral form, steps[k - 1] in the strided one."""
    steps = _i32([0, 2, 7, 9, 10, 11, 12])
    k, npos = 3, 6
    i = 5 if form == "ancestral" else 9
    j = i - 1 if form == "ancestral" else 7
    x, cur_i, cur_k = D.out(), _ctr(i), _ctr(k)
    x[:NUMEL] = 3.0                                      # the state the step wrote: replaced where m == 1
    strided = form == "strided"
    L.cdm_mask_blend(_p(x), None, NUMEL, _p(D.zero), _p(D.ones), NUMEL, _p(cur_i), _p(cur_k) if strided else None,
                     _p(steps) if strided else None, npos, TT, _p(D.t0), _p(D.t1), None, NUMEL, fresh, SEED,
                     _p(D.zseed), None, None, _s())
    got = _take(x, NUMEL)
    _is_draw(got, D.gen(KEY ^ R.KNOWN_NOISE_DOMAIN, j if fresh else 0), "xi")
    assert not np.array_equal(got, D.gen(KEY, j if fresh else 0)), "the plain key"


def _jump(L, D, k, j, fb, masked, fresh):
    land = torch.full((TT + 1,), j, dtype=torch.int32, device="cuda")
    fbt = torch.full((TT + 1,), float(fb), device="cuda")
    x, cur_k = D.out(), _ctr(k)
    x[:NUMEL] = 0.0
    L.cdm_mask_blend_jump(_p(x), None, NUMEL, _p(D.zero) if masked else None, _p(D.ones) if masked else None,
                          NUMEL if masked else 0, _p(cur_k), _p(land), TT, TT, _p(D.t0) if masked else None,
                          _p(D.t1) if masked else None, _p(D.t0), _p(fbt), None, NUMEL, fresh, None, NUMEL, SEED,
                          _p(D.zseed), None, None, _s())
    return _take(x, NUMEL)


@pytest.mark.parametrize("fresh", [1, 0])
def test_mask_blend_jump_xi_draws_domain_and_position(L, D, fresh):
    """No jump (fb = 0), landing level j = 6 at the position p = 3: xi = Philox(key ^ KNOWN_NOISE_DOMAIN, stream
    fresh ? p : 0), by position and not by level."""
    p, j = 3, 6
    got = _jump(L, D, p, j, 0.0, True, fresh)
    _is_draw(got, D.gen(KEY ^ R.KNOWN_NOISE_DOMAIN, p if fresh else 0), "xi of the jump form")
    assert not np.array_equal(got, D.gen(KEY ^ R.KNOWN_NOISE_DOMAIN, j)), "keyed by the level"


@pytest.mark.parametrize("masked", [False, True])
def test_mask_blend_jump_zeta_draws_domain_and_position(L, D, masked):
    """fa = 0, fb = 1 stores zeta = Philox(key ^ JUMP_NOISE_DOMAIN, stream p), with and without a blend in front (the
    blend's xi is multiplied by fa = 0)."""
    p = 3
    got = _jump(L, D, p, 6, 1.0, masked, 1)
    _is_draw(got, D.gen(KEY ^ R.JUMP_NOISE_DOMAIN, p), "zeta")
    assert not np.array_equal(got, D.gen(KEY ^ R.KNOWN_NOISE_DOMAIN, p)), "xi's domain"


def test_the_draws_of_one_run_are_disjoint(D):
    """z by timestep, z by position, xi and zeta of one run key at one stream id are four different streams."""
    s = [D.gen(k, 3) for k in (KEY, KEY ^ R.STEP_NOISE_DOMAIN, KEY ^ R.KNOWN_NOISE_DOMAIN, KEY ^ R.JUMP_NOISE_DOMAIN)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(s[a], s[b])


def test_flow_probe_is_the_oracle_uniform_against_half(L):
    """v[b][e] = (element e of the uniform stream under key ^ FLOW_PROBE_DOMAIN, sub = p) < 0.5 ? 1 : -1, the same in
    every row; H = 5, so H H = 25 is not a multiple of 4.  No transcendental: straight against the oracle."""
    n, H, p, npos = 3, 5, 4, 6
    v = torch.full((n * H * H + PAD,), float(SENT), device="cuda")
    cur, zs = _ctr(p), torch.tensor([SEED_DEV], dtype=torch.int64, device="cuda")
    L.cdm_flow_probe(_p(v), n, H, _p(cur), npos, SEED, _p(zs), _s())
    got = _take(v, n * H * H).reshape(n, H * H)

    def want(key, sub):
        return np.where(_ref_u01(H * H, key, sub) < np.float32(0.5), np.float32(1), np.float32(-1))
    for b in range(n):
        _same_bits(got[b], want(KEY ^ R.FLOW_PROBE_DOMAIN, p), f"row {b}")
    assert not np.array_equal(got[0], want(KEY, p)) and not np.array_equal(got[0], want(KEY ^ R.FLOW_PROBE_DOMAIN, p + 1))


# ------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------
def test_generator_argument_checks(L):
    """hipErrorInvalidValue with nothing launched (the sentinel-filled buffers stay intact): out null with n > 0, n < 0,
    randint hi < lo or a range beyond an int, uniform with a non-finite bound or hi < lo.  n == 0 returns 0 and writes
    nothing, with or without a buffer."""
    f, i = _buf(16), _buf(16, torch.int32)
    normal, uniform, randint = (L.raw("cdm_philox_" + k) for k in ("normal", "uniform", "randint"))
    inf, nan = float("inf"), float("nan")
    assert normal(None, 4, 1, 0, None, _s()) == INVALID
    assert normal(_p(f), -1, 1, 0, None, _s()) == INVALID
    assert uniform(None, 4, 0.0, 1.0, 1, 0, None, _s()) == INVALID
    assert uniform(_p(f), -1, 0.0, 1.0, 1, 0, None, _s()) == INVALID
    for lo, hi in ((1.0, 0.0), (nan, 1.0), (0.0, nan), (-inf, 1.0), (0.0, inf), (inf, inf), (-inf, -inf)):
        assert uniform(_p(f), 4, lo, hi, 1, 0, None, _s()) == INVALID, (lo, hi)
    assert randint(None, 4, 1, 10, 1, 0, None, _s()) == INVALID
    assert randint(_p(i), -1, 1, 10, 1, 0, None, _s()) == INVALID
    for lo, hi in ((2, 1), (1, 0), (0, -1), (2 ** 31 - 1, -2 ** 31), (0, 2 ** 31 - 1), (-2 ** 31, 2 ** 31 - 1)):
        assert randint(_p(i), 4, lo, hi, 1, 0, None, _s()) == INVALID, (lo, hi)
    for out in (_p(f), None):
        assert normal(out, 0, 1, 0, None, _s()) == 0
        assert uniform(out, 0, 0.0, 1.0, 1, 0, None, _s()) == 0
    for out in (_p(i), None):
        assert randint(out, 0, 1, 10, 1, 0, None, _s()) == 0
    torch.cuda.synchronize()
    assert (f == SENT).all() and (i == SENT).all(), "a refused or empty call wrote something"
    # the valid neighbours: lo == hi, and the widest range an int holds
    assert uniform(_p(f), 4, 0.5, 0.5, 1, 0, None, _s()) == 0
    assert randint(_p(i), 4, 1, 2 ** 31 - 1, 1, 0, None, _s()) == 0
    assert (_take(f, 16)[:4] == 0.5).all() and (f[4:] == SENT).all()
    t = i.cpu().numpy()
    assert np.array_equal(t[:4], R.randint_stream(4, 1, 2 ** 31 - 1, 1, 0)) and (t[4:] == SENT).all()
