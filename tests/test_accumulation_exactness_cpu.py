"""CPU: the exactness statement the blend backward's float64 accumulation rests on (csrc/blend_common.h, kGG).

The default backward adds a Gaussian's float32 per-tile parts with float64 atomics in whatever order the tiles arrive; the
fixed-order mode ("deterministic_backward") adds the same parts in list order.  A float64 sum of k float32 parts is exact -- so the
same bits for every order -- while the parts' exponent span plus log2(k) fits in 29 bits (24 mantissa bits + span + log2 k <= 53).
The GPU tests' allowance for "rounding-boundary flips" (tests/parity.py same_accumulation) only covers sums past that bound."""
import math

import numpy as np


def _parts(rng, k, span, base_exp=-20):
    """k float32 values of random sign and full 24-bit mantissas whose binary exponents cover exactly [base_exp, base_exp + span]."""
    mant = rng.integers(1 << 23, 1 << 24, size=k).astype(np.float64)
    exps = rng.integers(0, span + 1, size=k)
    exps[0], exps[1] = 0, span
    sign = rng.choice([-1.0, 1.0], size=k)
    v = np.array([math.ldexp(s * m, int(e) + base_exp - 24) for s, m, e in zip(sign, mant, exps)], np.float64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)      # representable in float32, exactly
    return v.astype(np.float32)


def _span(p):
    e = np.frexp(p.astype(np.float64))[1]
    return int(e.max() - e.min())


def _sum64(p, order):
    acc = 0.0
    for x in p[order]:
        acc += float(x)                 # float64 += float32 part, as the atomics and k_det_reduce do
    return acc


def test_float64_sums_of_float32_parts_within_the_bound_are_order_independent():
    rng = np.random.default_rng(11)
    for k, span in ((2, 28), (16, 25), (64, 23), (1000, 19), (4096, 17)):
        p = _parts(rng, k, span)
        assert _span(p) + math.ceil(math.log2(k)) <= 29, (k, _span(p))
        exact = math.fsum(float(x) for x in p)           # correctly rounded; equal to the exact sum iff the sum is representable
        ref = _sum64(p, np.arange(k))
        assert ref == exact, (k, span)
        for _ in range(40):
            s = _sum64(p, rng.permutation(k))
            assert s == ref, (k, span, s, ref)
            assert np.float32(s) == np.float32(ref)


def test_past_the_bound_two_orders_can_give_different_bits():
    rng = np.random.default_rng(12)
    k, span = 2000, 45                                       # 45 + 11 > 29: the sums round
    p = _parts(rng, k, span)
    sums = {_sum64(p, rng.permutation(k)) for _ in range(40)}
    assert len(sums) > 1, "expected order-dependent float64 sums past the exactness bound"
    # ... and the spread is a few float64 ulps of the summed magnitudes, far below a float32 ulp of them: the float32 results
    # differ only where a float32 rounding boundary falls between the float64 sums
    mag = float(np.abs(p.astype(np.float64)).sum())
    assert max(sums) - min(sums) <= k * 2.0 ** -52 * mag
