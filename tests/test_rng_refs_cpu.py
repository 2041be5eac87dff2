"""Holds the host RNG oracle (tests/_rng_ref.py) to account, on the CPU: the Random123 known answers of Philox4x32-10,
the properties of u01, the key-domain constants, and the statistics that make the oracle a credible generator (so the
GPU tests need only bit-equality with it).  Also the normal bound of tests/test_gpu_rng.py, checked on a pure-numpy fp32
restatement of box_muller.

Statistical bars are six standard errors of the statistic under the null hypothesis (uniform on (0, 1], or standard
normal), n = 2^20:
  mean of uniforms      sd 1 / sqrt(12 n)            variance of uniforms   sd sqrt((1/80 - 1/144) / n)
  chi-square, 256 bins  mean 255, sd sqrt(2 * 255)   correlation            sd 1 / sqrt(n)
  mean of normals       sd 1 / sqrt(n)               variance of normals    sd sqrt(2 / n)
  kurtosis of normals   sd sqrt(96 / n)  (Var of the fourth moment of N(0,1): E z^8 - (E z^4)^2 = 105 - 9)
"""
import numpy as np
import pytest

import _rng_ref as R

N = 1 << 20
SEED = 0x1234_5678_9ABC_DEF0

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(v) for v in R.philox(*ctr, *key))
    assert got == want, " ".join(f"{v:08x}" for v in got)


def test_philox_is_vectorised_elementwise():
    """An array call equals the scalar calls, whichever arguments are arrays (the three known answers in one call)."""
    cols = list(zip(*[c + k for c, k, _ in KAT]))
    got = np.stack(R.philox(*(np.array(c, dtype=np.uint64) for c in cols)), axis=1)
    assert got.dtype == np.uint32 and got.tolist() == [list(w) for _, _, w in KAT]
    q = np.arange(5, dtype=np.uint64)
    many = np.stack(R.philox(q, 0, 7, 0x5EED, 1, 2), axis=1)
    for i in range(5):
        assert many[i].tolist() == [int(v) for v in R.philox(i, 0, 7, 0x5EED, 1, 2)]


def _u_of_m(m):
    return R.u01(np.asarray(m, dtype=np.uint64).astype(np.uint32) << np.uint32(8))


def test_u01_lower_half_is_exact():
    """Every m < 2^23: (m + 0.5) has 24 significant bits, so u01 is (m + 0.5) / 2^24 exactly."""
    m = np.arange(1 << 23, dtype=np.uint32)
    u = _u_of_m(m)
    assert u.dtype == np.float32
    assert np.array_equal(u.astype(np.float64), (m.astype(np.float64) + 0.5) / 2.0 ** 24)


def test_u01_upper_half_rounds_ties_to_even():
    """Every m >= 2^23: m + 0.5 is a tie between m and m + 1 and goes to the even one."""
    m = np.arange(1 << 23, 1 << 24, dtype=np.uint32)
    u = _u_of_m(m)
    even = (m + (m & np.uint32(1))).astype(np.float64)
    assert np.array_equal(u.astype(np.float64), even / 2.0 ** 24)


def test_u01_range_edges_and_low_bits():
    m = np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1], dtype=np.uint32)
    u = _u_of_m(m)
    assert u.min() == np.float32(2.0 ** -25) and u[0] == u.min()
    assert u.max() == np.float32(1.0) and u[-1] == np.float32(1.0) and u[-2] < np.float32(1.0)
    want = [2.0 ** -25, 1.5 * 2.0 ** -24, 0.5 - 2.0 ** -25, 0.5, 0.5 + 2.0 ** -23, 1.0 - 2.0 ** -23, 1.0]
    assert u.astype(np.float64).tolist() == want
    assert np.all(u > 0)
    # the low 8 bits of the word do not enter
    assert np.array_equal(R.u01(np.array([0x12345600, 0x123456FF], dtype=np.uint32))[:1],
                          R.u01(np.array([0x123456FF], dtype=np.uint32)))


def test_u01_is_monotone():
    rng = np.random.default_rng(1)
    m = np.sort(np.concatenate([rng.integers(0, 1 << 24, 1 << 20), np.arange((1 << 24) - 4096, 1 << 24),
                                np.arange((1 << 23) - 2048, (1 << 23) + 2048)])).astype(np.uint32)
    u = _u_of_m(m)
    assert np.all(np.diff(u) >= 0)


def test_find_u_one_reproduces_the_known_words():
    """Streams of the uniform domain whose element `word` is exactly 1.0f: what cdm_context_drop's p_drop = 1 case and
    the device test of u01's upper edge are built on."""
    hits0 = R.find_u_one(0, R.UNIFORM_C3, 1_600_000)
    assert (1543363, 0) in hits0 and (674387, 1) in hits0
    hits1 = R.find_u_one(1234, R.UNIFORM_C3, 20_300_000, min_sub=18_000_000)     # (key 1234 has no hit below this one)
    assert (20278353, 3) in hits1
    for seed, hits in ((0, hits0), (1234, hits1)):
        for sub, j in hits:
            a, b = R.uniform_stream(4, 0.0, 1.0, seed, sub)
            assert a[j] == np.float32(1.0) and b[j] == np.float32(1.0)
            assert R.uniform_words(4, seed, sub)[j] >> 8 == 0xFFFFFF


def test_domain_constants_spell_their_names():
    for name, value in R.DOMAINS.items():
        assert value.to_bytes(8, "big").decode("ascii") == name
    assert len(set(R.DOMAINS.values())) == 4
    assert R.DOMAINS == {"pos_step": R.STEP_NOISE_DOMAIN, "known_xi": R.KNOWN_NOISE_DOMAIN,
                         "jumpzeta": R.JUMP_NOISE_DOMAIN, "flowprob": R.FLOW_PROBE_DOMAIN}
    assert len({R.NORMAL_C3, R.UNIFORM_C3, R.RANDINT_C3}) == 3


def test_uniform_stream_forms():
    """At (0, 1) both forms are u01 of the words.  At (-1, 1) they coincide as well: hi - lo = 2 is a power of two, so the
    product is exact and there is one rounding either way.  At +-1/sqrt(2) (model.py's init bound for two input channels)
    they differ somewhere, by at most one ulp of 1.  Every value stays inside [lo, hi]."""
    w = R.uniform_words(4099, SEED, 5)
    a, b = R.uniform_stream(4099, 0.0, 1.0, SEED, 5)
    assert np.array_equal(a, R.u01(w)) and np.array_equal(a, b)
    a, b = R.uniform_stream(4099, -1.0, 1.0, SEED, 5)
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, b) and a.min() >= -1 and a.max() <= 1
    bound = np.float32(1.0 / np.sqrt(2.0))
    c, d = R.uniform_stream(4099, -bound, bound, SEED, 5)
    assert np.any(c != d) and np.abs(c.astype(np.float64) - d).max() <= 2.0 ** -24
    for v in (c, d):
        assert v.min() >= -bound and v.max() <= bound
    # a prefix of a longer stream, whatever n % 4
    for n in (1, 3, 4, 5):
        assert np.array_equal(R.uniform_stream(n, -1.0, 1.0, SEED, 5)[0], a[:n])


def test_randint_stream_range_and_words():
    for lo, hi in ((1, 1500), (0, 0), (-5, 5), (1, 2 ** 31 - 1)):
        t = R.randint_stream(4096, lo, hi, SEED, 1 << 24)
        assert t.dtype == np.int32 and t.min() >= lo and t.max() <= hi
    x, y, _, _ = R.philox(3, 0x71, 1 << 24, 0xA11C, *R.key_words(SEED))
    assert int(R.randint_stream(4, 1, 1500, SEED, 1 << 24)[3]) == 1 + ((int(x) << 32) | int(y)) % 1500
    t = R.randint_stream(N, 1, 16, SEED, 1 << 24)
    chi = ((np.bincount(t, minlength=17)[1:] - N / 16) ** 2 / (N / 16)).sum()
    assert chi < 15 + 6 * np.sqrt(30)


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def _u(seed, sub):
    return R.uniform_stream(N, 0.0, 1.0, seed, sub)[0].astype(np.float64)


def test_uniform_statistics():
    u = _u(SEED, 3 << 24)
    assert abs(u.mean() - 0.5) < 6 / np.sqrt(12 * N)
    assert abs(u.var() - 1 / 12) < 6 * np.sqrt((1 / 80 - 1 / 144) / N)
    counts = np.bincount(np.minimum((u * 256).astype(np.int64), 255), minlength=256)
    chi = ((counts - N / 256) ** 2 / (N / 256)).sum()
    print(f"uniform: mean {u.mean():.6f} var {u.var():.6f} chi2(255) {chi:.1f}")
    assert chi < 255 + 6 * np.sqrt(2 * 255)


def test_streams_keys_and_domains_are_uncorrelated():
    bar = 6 / np.sqrt(N)
    base = _u(SEED, 3 << 24)
    others = {"sub + 1": _u(SEED, (3 << 24) + 1), "key ^ 1": _u(SEED ^ 1, 3 << 24),
              "key ^ high bit": _u(SEED ^ (1 << 32), 3 << 24),
              "two key domains": _u(SEED ^ R.STEP_NOISE_DOMAIN, 3 << 24)}
    for what, v in others.items():
        c = _corr(base, v)
        print(f"{what}: corr {c:+.2e} (bar {bar:.2e})")
        assert abs(c) < bar, what
        assert not np.array_equal(base, v)
    a = _u(SEED ^ R.KNOWN_NOISE_DOMAIN, 7)
    b = _u(SEED ^ R.JUMP_NOISE_DOMAIN, 7)
    assert abs(_corr(a, b)) < bar
    # the uniform and the normal domain words give different words for one (key, counter)
    assert not np.array_equal(R._quad_words(64, SEED, 7, R.UNIFORM_C3), R._quad_words(64, SEED, 7, R.NORMAL_C3))
    # lag-1 within a stream, and the four words of a counter against each other
    assert abs(_corr(base[:-1], base[1:])) < bar
    q = base.reshape(-1, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(_corr(q[:, i], q[:, j])) < 6 / np.sqrt(N / 4)


def test_normal_statistics():
    z, r = R.normal_stream64(N, SEED, 3 << 24)
    assert z.shape == (N,) and r.shape == (N,) and np.all(np.abs(z) <= r)
    m, v = z.mean(), z.var()
    kurt = ((z - m) ** 4).mean() / v ** 2
    print(f"normal: mean {m:+.2e} var {v:.6f} kurtosis {kurt:.4f}")
    assert abs(m) < 6 / np.sqrt(N)
    assert abs(v - 1) < 6 * np.sqrt(2 / N)
    assert abs(kurt - 3) < 6 * np.sqrt(96 / N)
    # cos / sin of one pair, the two pairs of a counter, and the next stream
    q = z.reshape(-1, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(_corr(q[:, i], q[:, j])) < 6 / np.sqrt(N / 4)
    z2, _ = R.normal_stream64(N, SEED, (3 << 24) + 1)
    assert abs(_corr(z, z2)) < 6 / np.sqrt(N)
    # a prefix of a longer stream, whatever n % 4; r is shared by the two elements of a pair
    for n in (1, 3, 5, 1027):
        zs, rs = R.normal_stream64(n, SEED, 3 << 24)
        assert np.array_equal(zs, z[:n]) and np.array_equal(rs, r[:n])
    assert np.array_equal(r[0::4], r[1::4]) and np.array_equal(r[2::4], r[3::4])


def _word_of_u(u):
    """a word whose u01 is u (u = (m + 0.5) 2^-24 for m < 2^23, an even multiple of 2^-24 above)"""
    m = int(u * 2 ** 24 - 0.5) if u < 0.5 else min(int(u * 2 ** 24), (1 << 24) - 1)
    w = np.uint32(m << 8)
    assert float(R.u01(np.array([w]))[0]) == u, u
    return w


def test_box_muller_fp32_restatement_within_the_device_bound():
    """numpy's fp32 log / sqrt / sin / cos in box_muller's order against the fp64 oracle, per element within
    B = r (4 pi + 10) U + 2 U (tests/test_gpu_rng.py's bound for the device), over 2^22 random word pairs and every
    combination of the edge values u1 in {2^-25, 1} (r largest, r = 0) and u2 in {2^-25, 0.5, 1} (the angle's ends and
    pi).  Measured here: 0.41 of the tighter r (4 pi + 4) U + 2 U."""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32)
    e1 = [_word_of_u(u) for u in (2.0 ** -25, 1.0)]
    e2 = [_word_of_u(u) for u in (2.0 ** -25, 0.5, 1.0)]
    ea = np.array([x for x in e1 for _ in e2] + [x for x in e1] * 2, dtype=np.uint32)
    eb = np.array([y for _ in e1 for y in e2] + [b[0], b[0], b[1], b[1]], dtype=np.uint32)
    a, b = np.concatenate([ea, a]), np.concatenate([eb, b])
    c64, s64, r = R.box_muller64(a, b)
    c32, s32 = R.box_muller32(a, b)
    assert c32.dtype == np.float32 and s32.dtype == np.float32
    assert np.isfinite(c32).all() and np.isfinite(s32).all()
    err = np.maximum(np.abs(c32.astype(np.float64) - c64), np.abs(s32.astype(np.float64) - s64))
    ratio, tight = (err / R.normal_bound(r)).max(), (err / R.normal_bound(r, 4.0)).max()
    print(f"fp32 restatement: max |z - z64| / B = {ratio:.3f}; against r (4 pi + 4) U + 2 U: {tight:.3f}")
    assert ratio <= 1.0
    assert tight <= 1.0
    # u1 = 1: r = 0 and both values are zero; u1 = 2^-25: the largest |z| a draw can have
    one = a == e1[1]
    assert np.all(r[one] == 0) and np.all(c32[one] == 0) and np.all(s32[one] == 0)
    assert abs(r.max() - np.sqrt(50 * np.log(2.0))) < 1e-12
