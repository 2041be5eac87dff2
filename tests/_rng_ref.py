"""Host oracle of the device RNG (csrc/sampler_parts.h: philox, u01, box_muller): numpy only, no torch device.

Every random number the device makes is a function of (key, counter) through Philox4x32-10, then u01, then (for the
normal draws) Box-Muller.  This file restates the three and the streams built on them, so that the device can be held to
something other than itself; tests/test_rng_refs_cpu.py holds this file to the Random123 known answers and to the
statistics a generator must have.

  counter words                      c0        c1       c2    c3
  cdm_philox_normal / in-kernel z    q         q >> 32  sub   0x5EED    element e = 4 q + j, j = word pair / cos, sin
  cdm_philox_uniform / u01 element   q         q >> 32  sub   0x0417    element e = 4 q + j, j = the word
  cdm_philox_randint                 i         0x71     sub   0xA11C    one counter per element, words x and y
  key words                          k0 = (uint32)seed, k1 = seed >> 32
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
U = 2.0 ** -24                      # fp32 unit roundoff

NORMAL_C3 = 0x5EED
UNIFORM_C3 = 0x0417
RANDINT_C1, RANDINT_C3 = 0x71, 0xA11C

# key domains: XORed into the run key seed ^ *seed_dev; each is the big-endian ASCII of its name
STEP_NOISE_DOMAIN = 0x706F735F73746570      # "pos_step": z of cdm_ddim_step_pos / cdm_ddim_step_guided, stream k
KNOWN_NOISE_DOMAIN = 0x6B6E6F776E5F7869     # "known_xi": xi of cdm_mask_blend / cdm_mask_blend_jump
JUMP_NOISE_DOMAIN = 0x6A756D707A657461      # "jumpzeta": zeta of cdm_mask_blend_jump, stream p
FLOW_PROBE_DOMAIN = 0x666C6F7770726F62      # "flowprob": the Rademacher probes of the flow likelihood, stream p
DOMAINS = {"pos_step": STEP_NOISE_DOMAIN, "known_xi": KNOWN_NOISE_DOMAIN, "jumpzeta": JUMP_NOISE_DOMAIN,
           "flowprob": FLOW_PROBE_DOMAIN}

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & M32


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10, vectorised: every argument a scalar or an array of 32-bit words (broadcast); four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(a) for a in (c0, c1, c2, c3, k0, k1)))
    m0, m1, w0, w1 = (np.uint64(v) for v in (PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1))
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits: no overflow of uint64
        n0 = (p1 >> s32) ^ c1 ^ k0
        n2 = (p0 >> s32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def key_words(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def u01(v):
    """The kernel's fp32 operations: ((float)(v >> 8) + 0.5f) * 2^-24.  Range (0, 1]: for v >> 8 >= 2^23 the + 0.5f is a
    tie and rounds to even, so the all-ones mantissa gives exactly 1.0f.  Never 0."""
    m = (np.asarray(v, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)        # < 2^24: exact
    return (m + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def _quad_words(n, seed, sub, c3):
    """The words of counters q = 0 .. ceil(n / 4) - 1 as [nq, 4] (the high counter word q >> 32 is 0 below 2^34 elements)."""
    nq = (int(n) + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    k0, k1 = key_words(seed)
    return np.stack(philox(q & M32, q >> np.uint64(32), int(sub) & 0xFFFFFFFF, c3, k0, k1), axis=1)


def uniform_words(n, seed, sub):
    return _quad_words(n, seed, sub, UNIFORM_C3).reshape(-1)[:int(n)]


def uniform_stream(n, lo, hi, seed, sub):
    """What cdm_philox_uniform(out, n, lo, hi, seed, sub) writes: out = lo + (hi - lo) * u01 in fp32.  The compiler may
    contract the product and the sum into one fma, so both are returned: (two roundings, one rounding).  hi - lo is one
    fp32 rounding in both.  The one-rounding form is evaluated in fp64 and rounded once; the fp64 sum is checked to be
    exact (TwoSum), so that rounding is the fma's.  At (0, 1) both are u01 itself."""
    u = u01(uniform_words(n, seed, sub))
    lo32, hi32 = np.float32(lo), np.float32(hi)
    d = np.float32(hi32 - lo32)
    two = lo32 + d * u
    p = np.float64(d) * u.astype(np.float64)                # 24 x 24 bits: exact
    s = np.float64(lo32) + p
    bb = s - np.float64(lo32)
    err = (np.float64(lo32) - (s - bb)) + (p - bb)          # TwoSum: lo + p == s + err exactly
    if np.any(err != 0):
        raise ValueError("lo + (hi - lo) u is not exact in fp64 for this (lo, hi): the one-rounding form needs more bits")
    return two.astype(np.float32), s.astype(np.float32)


def randint_stream(n, lo, hi, seed, sub):
    """What cdm_philox_randint writes: lo + (((x << 32) | y) % (hi - lo + 1)), counter (i, 0x71, sub, 0xA11C)."""
    i = np.arange(int(n), dtype=np.uint64)
    k0, k1 = key_words(seed)
    x, y, _, _ = philox(i, RANDINT_C1, int(sub) & 0xFFFFFFFF, RANDINT_C3, k0, k1)
    r = (x.astype(np.uint64) << np.uint64(32)) | y.astype(np.uint64)
    return (np.int64(lo) + (r % np.uint64(int(hi) - int(lo) + 1)).astype(np.int64)).astype(np.int32)


def box_muller64(a, b):
    """fp64 Box-Muller of the word pair (a, b): u1, u2 the fp32 u01 of the words (restated exactly), everything after in
    fp64 with the angle 2 pi u2.  Returns (r cos, r sin, r), r = sqrt(-2 ln u1)."""
    u1, u2 = u01(a).astype(np.float64), u01(b).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return r * np.cos(ang), r * np.sin(ang), r


def box_muller32(a, b):
    """The kernel's box_muller restated with numpy's fp32 log / sqrt / sin / cos (another libm than the device's)."""
    u1, u2 = u01(a), u01(b)
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    ang = np.float32(6.283185307179586) * u2
    return r * np.cos(ang), r * np.sin(ang)


def normal_bound(r, c=10.0):
    """|z - z64| <= r (4 pi + c) U + 2 U.  r 4 pi U: two roundings of an angle up to 2 pi (the fp32 2 pi and the
    product); c = 10: 4 for a two-ulp sincosf at magnitude 1, the rest a one-ulp logf (through the sqrt: half), a
    one-ulp sqrtf and the final product; 2 U absolute for the results near zero."""
    return r * (4.0 * np.pi + c) * U + 2.0 * U


def normal_stream64(n, seed, sub):
    """fp64 values of what cdm_philox_normal(out, n, seed, sub) writes, and r per element: element 4 q + 0 / 1 is
    r cos / r sin of the words (x, y) of counter q, 4 q + 2 / 3 of (z, w)."""
    w = _quad_words(n, seed, sub, NORMAL_C3)
    c0, s0, r0 = box_muller64(w[:, 0], w[:, 1])
    c1, s1, r1 = box_muller64(w[:, 2], w[:, 3])
    z = np.stack([c0, s0, c1, s1], axis=1).reshape(-1)[:int(n)]
    r = np.stack([r0, r0, r1, r1], axis=1).reshape(-1)[:int(n)]
    return z, r


def find_u_one(seed, domain_c3, max_sub, min_sub=0, chunk=1 << 21):
    """Every (sub, word) with min_sub <= sub < max_sub whose word of counter (0, 0, sub, domain_c3) under the key `seed`
    has v >> 8 == 0xFFFFFF, i.e. u01 == 1.0f exactly; element `word` of that stream is the hit.  Ascending in sub."""
    k0, k1 = key_words(seed)
    hits = []
    for s0 in range(int(min_sub), int(max_sub), chunk):
        sub = np.arange(s0, min(s0 + chunk, int(max_sub)), dtype=np.uint64)
        for j, w in enumerate(philox(0, 0, sub, domain_c3, k0, k1)):
            for i in np.nonzero((w >> np.uint32(8)) == np.uint32(0xFFFFFF))[0]:
                hits.append((int(sub[i]), j))
    return sorted(hits)
