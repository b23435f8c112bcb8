"""CPU: the algebra behind nomad_amd/csrc/posconv_fft_f32.hip.h, step by step as the kernels do it.

One group of the pos-conv is the 128-tap correlation C[t] = sum_k A[t + k] V[k] over the zero-padded frames of a clip.  The engine
cuts a clip into units of 385 output frames (overlap-save, N = 512), packs two real channels into one complex 512-point transform,
takes the two half spectra apart, multiplies every bin by the real embedding [[Wr, -Wi], [Wi, Wr]] of W = conj(DFT(V)) / 512, puts
the packed spectrum together again and reads the inverse transform off a forward one at index (512 - t) mod 512.  This file
restates those steps in float64 - the column layout of the spectra included - and holds them to the direct correlation.
"""
import torch

N, BLK, BINS = 512, 385, 257


def _col(ch, part):
    """column of channel ch (0 .. 47), part 0 = real / 1 = imaginary, in a row of the spectrum"""
    return (ch // 16) * 32 + part * 16 + ch % 16


def _weights(v):
    """v [48 out][128 taps][48 in] -> [257][96][96] ([bin][output column][input column])"""
    k = torch.arange(128, dtype=torch.float64)
    f = torch.arange(BINS, dtype=torch.float64)
    ang = 2 * torch.pi * f[:, None] * k[None, :] / N
    wr = torch.einsum("fk,nkc->fnc", torch.cos(ang), v) / N
    wi = torch.einsum("fk,nkc->fnc", torch.sin(ang), v) / N
    wf = torch.zeros(BINS, 96, 96, dtype=torch.float64)
    for n in range(48):
        for c in range(48):
            wf[:, _col(n, 0), _col(c, 0)] = wr[:, n, c]
            wf[:, _col(n, 0), _col(c, 1)] = -wi[:, n, c]
            wf[:, _col(n, 1), _col(c, 0)] = wi[:, n, c]
            wf[:, _col(n, 1), _col(c, 1)] = wr[:, n, c]
    return wf


def _unit(frames, wf):
    """frames [512][48] (one unit's input, zeros behind the clip) -> [512][48]: the circular correlation"""
    z = torch.complex(frames[:, 0::2], frames[:, 1::2])          # channel pair (2 p, 2 p + 1) is transform p
    Z = torch.fft.fft(z, dim=0)
    Zn = Z[(N - torch.arange(BINS)) % N]
    Z = Z[:BINS]
    X = torch.zeros(BINS, 96, dtype=torch.float64)
    for p in range(24):
        X[:, _col(2 * p, 0)] = 0.5 * (Z[:, p].real + Zn[:, p].real)
        X[:, _col(2 * p + 1, 0)] = 0.5 * (Z[:, p].imag + Zn[:, p].imag)
        X[:, _col(2 * p, 1)] = 0.5 * (Z[:, p].imag - Zn[:, p].imag)
        X[:, _col(2 * p + 1, 1)] = 0.5 * (Zn[:, p].real - Z[:, p].real)
    Y = torch.einsum("fk,fnk->fn", X, wf)
    W = torch.zeros(N, 24, dtype=torch.complex128)
    for p in range(24):
        re0, re1, im0, im1 = (Y[:, _col(2 * p, 0)], Y[:, _col(2 * p + 1, 0)], Y[:, _col(2 * p, 1)], Y[:, _col(2 * p + 1, 1)])
        W[:BINS, p] = torch.complex(re0 - im1, im0 + re1)
        W[N - torch.arange(1, N // 2), p] = torch.complex(re0 + im1, re1 - im0)[1:N // 2]
    out = torch.fft.fft(W, dim=0)[(N - torch.arange(N)) % N]     # the 1 / 512 is in the weights
    res = torch.zeros(N, 48, dtype=torch.float64)
    res[:, 0::2], res[:, 1::2] = out.real, out.imag
    return res


def test_overlap_save_units_equal_the_direct_correlation():
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(48, 128, 48, generator=gen, dtype=torch.float64)
    wf = _weights(v)
    for T in (1, 199, 385, 386, 771):
        x = torch.zeros(T + 128, 48, dtype=torch.float64)
        x[64:64 + T] = torch.randn(T, 48, generator=gen, dtype=torch.float64)
        ref = torch.stack([torch.einsum("kc,nkc->n", x[t:t + 128], v) for t in range(T)])
        got = []
        for j in range((T + BLK - 1) // BLK):
            frames = torch.zeros(N, 48, dtype=torch.float64)
            have = x[BLK * j:BLK * j + N]
            frames[:len(have)] = have
            got.append(_unit(frames, wf)[:min(BLK, T - BLK * j)])
        got = torch.cat(got)
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < 1e-10 * max(1.0, ref.abs().max().item()), T


def test_octal_digit_reversal_is_where_the_in_place_transform_leaves_a_bin():
    """Three radix-8 decimation-in-frequency stages, in place: bin k ends at the position with k's octal digits reversed."""
    gen = torch.Generator().manual_seed(4)
    x = torch.complex(torch.randn(N, generator=gen, dtype=torch.float64), torch.randn(N, generator=gen, dtype=torch.float64))
    buf = x.clone()
    r = torch.arange(8, dtype=torch.float64)
    dft8 = torch.exp(-2j * torch.pi * r[:, None] * r[None, :] / 8)
    for stage in range(3):
        span = N >> (3 * stage)
        step = span // 8
        for bf in range(64):
            blk, j = divmod(bf, step)
            idx = blk * span + j + step * torch.arange(8)
            buf[idx] = (dft8 @ buf[idx]) * torch.exp(-2j * torch.pi * j * r / span)
    k = torch.arange(N)
    rev = ((k & 7) << 6) | (k & 0x38) | (k >> 6)
    assert (buf[rev] - torch.fft.fft(x)).abs().max().item() < 1e-10
