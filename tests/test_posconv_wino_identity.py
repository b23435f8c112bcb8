"""CPU: the nested F(2,2) identity behind nomad_amd/csrc/posconv_wino_f32.hip.h.

A stride-1 correlation C[t] = sum_k A[t + k] V[k] with an even tap count, per tap pair j and output pair s:
    D0[r] = A[2r] - A[2r+1]     Z1[r] = A[2r+1]             D2[r] = A[2r+2] - A[2r+1]
    m1[s] = sum_j D0[s+j] V[2j]   m2[s] = sum_j Z1[s+j] (V[2j] + V[2j+1])   m3[s] = sum_j D2[s+j] V[2j+1]
    C[2s] = m1[s] + m2[s]       C[2s+1] = m2[s] + m3[s]
Each m is a correlation of the same kind at half the rate and half the taps, so the form nests: two levels compute the 128-tap
pos-conv from 9 quarter-rate 32-tap correlations, 9 / 16 of the products.  Frames behind the input's end stand for zeros (the
surplus outputs of a length that is no multiple of 4 are dropped).
"""
import numpy as np
import pytest


def direct(a, v, T):
    K = v.shape[0]
    return np.stack([sum(v[k] @ a[t + k] for k in range(K)) for t in range(T)])


def nested(a, v, T, levels, dtype=np.float64):
    """C[0 .. T) of the correlation of a [frames][cin] with v [taps][cout][cin]; operands and products in `dtype`, weight sums in
    float64 rounded once (as the engine forms them)."""
    K = v.shape[0]
    if levels == 0:
        a, v = a.astype(dtype), v.astype(dtype)
        out = np.zeros((T, v.shape[1]), dtype)
        for k in range(K):                       # one accumulator per output, taps in order
            out += a[k:k + T] @ v[k].T
        return out
    S = (T + 1) // 2
    need = 2 * (S + K // 2 - 1) + 1              # frames the half-rate operands read
    a = a.astype(dtype)
    if a.shape[0] < need:
        a = np.concatenate([a, np.zeros((need - a.shape[0], a.shape[1]), dtype)])
    n = S + K // 2 - 1
    d0 = a[0:2 * n:2] - a[1:2 * n:2]
    z1 = a[1:2 * n:2]
    d2 = a[2:2 * n + 1:2] - a[1:2 * n:2]
    m1 = nested(d0, v[0::2], S, levels - 1, dtype)
    m2 = nested(z1, v[0::2] + v[1::2], S, levels - 1, dtype)
    m3 = nested(d2, v[1::2], S, levels - 1, dtype)
    out = np.empty((2 * S, v.shape[1]), dtype)
    out[0::2] = m1 + m2
    out[1::2] = m2 + m3
    return out[:T]


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 9, 27])
def test_nested_form_equals_direct(T, levels):
    rng = np.random.default_rng(T + 100 * levels)
    taps = 16
    a = rng.standard_normal((T + taps, 6))       # T + taps - 1 frames are read by the direct form
    v = rng.standard_normal((taps, 5, 6))
    y = nested(a, v, T, levels)
    assert y.shape == (T, 5)
    np.testing.assert_allclose(y, direct(a, v, T), rtol=0, atol=1e-12)


@pytest.mark.parametrize("peaky", [False, True])
def test_fp32_error_of_two_levels_stays_within_the_bar(peaky):
    """The accuracy bar of tests/test_gpu_posconv_wino.py restated on the CPU: one pos-conv group on the seeded model's folded
    weights and inputs of the size the encoder feeds it, fp32 operands and accumulators against float64.  The nested form's
    error must stay below 2e-5 and within twice the direct form's + 1e-7."""
    import torch
    from nomad_amd.weights import seeded_state_dict
    sd = seeded_state_dict(1, qk_gain=6.0) if peaky else seeded_state_dict(0)
    v = sd["ssl_model.encoder.pos_conv.0.weight_v"].double()
    g = sd["ssl_model.encoder.pos_conv.0.weight_g"].double().view(128)
    w = (v * (g / v.pow(2).sum(dim=(0, 1)).sqrt())).float().numpy()[:48]          # group 0: [48 out][48 in][128]
    w = np.ascontiguousarray(w.transpose(2, 0, 1))                                 # [tap][out][in]
    rng = np.random.default_rng(3)
    T = 27
    a = np.zeros((T + 128, 48), np.float32)
    a[64:64 + T] = rng.standard_normal((T, 48)).astype(np.float32)                 # LayerNorm-scale features
    ref = direct(a.astype(np.float64), w.astype(np.float64), T)
    e_direct = np.abs(nested(a, w, T, 0, np.float32) - ref).max()
    e_nested = np.abs(nested(a, w.astype(np.float64), T, 2, np.float32) - ref).max()
    print("fp32 error against float64: direct", e_direct, "two levels", e_nested, "max |C|", np.abs(ref).max())
    assert e_nested < 2e-5 and e_direct < 2e-5
    assert e_nested <= 2 * e_direct + 1e-7
