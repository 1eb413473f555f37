"""CPU: the pass-1 IDCT folds of recon.hip (idct_1d<true>) equal the exact SSE2 transform
(idct_sse2.hpp:23-65, ref) whenever inputs 1-7 lie in the dequant clamp range [-2048, 2047]
(mb_decoder.cpp:146) and input 0 (QFS[0]: intra DC or the unclamped '1s' coefficient) is any int16.

The model (tests/directed_idct.py) is plain int64 numpy with explicit int16 wrap (slli) and saturation
(adds/subs); every folded product is asserted to stay below 2^31 (the kernel multiplies in 32 bits).
"""
import itertools

import numpy as np


from directed_idct import idct_1d  # the 1-D model, shared with the directed IDCT tests


def test_pass1_folds_equal_exact_transform_random():
    rng = np.random.default_rng(7)
    n = 1_000_000
    s = [rng.integers(-32768, 32768, n)] + [rng.integers(-2048, 2048, n) for _ in range(7)]
    assert np.array_equal(idct_1d(s, False), idct_1d(s, True))
    edge = np.array([-2048, -2047, -1, 0, 1, 2046, 2047])
    s = [rng.integers(-32768, 32768, n)] + [rng.choice(edge, n) for _ in range(7)]
    assert np.array_equal(idct_1d(s, False), idct_1d(s, True))


def test_pass1_folds_equal_exact_transform_corners():
    corners = np.array(list(itertools.product([-2048, 2047], repeat=7))).T
    s0 = np.repeat(np.arange(-32768, 32768, 97), corners.shape[1])
    c = np.tile(corners, (1, len(s0) // corners.shape[1]))
    out = idct_1d([s0] + list(c), False)
    assert np.array_equal(out, idct_1d([s0] + list(c), True))
    assert (np.abs(out) == 32767).any() or (out == -32768).any()  # the exact model does saturate here

