"""CPU: the polyphase Winograd identity behind nomad_amd/csrc/conv_s2_f32.hip.h, in float64.

A k = 3, stride 2 convolution y[t] = w0 x[2t] + w1 x[2t+1] + w2 x[2t+2] computed per output pair s as
    P = (w0 + w2) x[4s+2]
    y[2s]   = w0 (x[4s]   - x[4s+2]) + w1 x[4s+1] + P
    y[2s+1] = w2 (x[4s+4] - x[4s+2]) + w1 x[4s+3] + P
5 matrix products per pair instead of 6.  With an odd output count L the last pair has no odd output and reads frames up to 2L
only (the input has at least 2L + 1 frames).
"""
import numpy as np
import pytest


def direct(x, w):
    L = (x.shape[0] - 3) // 2 + 1
    return np.stack([w[0] @ x[2 * t] + w[1] @ x[2 * t + 1] + w[2] @ x[2 * t + 2] for t in range(L)])


def polyphase(x, w):
    L = (x.shape[0] - 3) // 2 + 1
    y = np.empty((L, w.shape[1]))
    for s in range((L + 1) // 2):
        p = (w[0] + w[2]) @ x[4 * s + 2]
        y[2 * s] = w[0] @ (x[4 * s] - x[4 * s + 2]) + w[1] @ x[4 * s + 1] + p
        if 2 * s + 1 < L:
            y[2 * s + 1] = w[2] @ (x[4 * s + 4] - x[4 * s + 2]) + w[1] @ x[4 * s + 3] + p
    return y


@pytest.mark.parametrize("lin", [3, 4, 5, 6, 7, 8, 21, 22, 603, 604])
def test_polyphase_equals_direct(lin):
    rng = np.random.default_rng(lin)
    x = rng.standard_normal((lin, 16))
    w = rng.standard_normal((3, 12, 16))
    L = (lin - 3) // 2 + 1
    y = polyphase(x, w)
    assert y.shape == (L, 12)
    np.testing.assert_allclose(y, direct(x, w), rtol=0, atol=1e-12)

