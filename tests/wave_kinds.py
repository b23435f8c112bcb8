"""Degenerate and product-like waveforms for the float64-held tests (``test_wave_kinds_host.py``, ``test_gpu_wave_kinds_f64.py``).
Imported by the tests like ``ref64``; not a test module itself.

Every other float64-held test feeds the network ``0.1 * randn``, clamped: zero-mean and white, its conv0 GroupNorm variance far
from both 0 and eps.  The kinds below are what an enhancement loss and the degradation sweeps feed it instead:

  silence        zeros                              variance exactly 0, rstd = 1 / sqrt(eps), identical rows everywhere
  constant       0.5 everywhere                     true variance 0 from a non-zero mean: the clamp, fp32 ``y - mean``
  dc_offset      0.5 + 1e-3 randn                   mean^2 / variance ~1e5
  faint          1e-4 randn                         variance << eps
  impulse        one sample = 1 at n // 2           one frame carries everything
  square         sign(sin(2 pi 220 t / 16000))      saturation, plateaus
  full_scale     randn.clamp(-1, 1)                 saturation
  int16          round(base * 32768) / 32768        quantised input
  hard_clipped   degrade_ref.clip(base, [40])       what ``degrade_clip`` feeds the forward
  noisy_m20db    degrade_ref.noise(base, randn, [-20])   amplitude above 1, what ``degrade_noise`` feeds it
  half_silent    base, second half zeroed           windows and frames over silence beside signal

with ``base = (0.1 * randn(n)).clamp(-1, 1)``, all from ONE seeded generator.

Geometries: ``N_SHORT`` (T = 65: crosses the 64-frame tiles; L0 = 4175: five statistics chunks of 1024 frames), ``N_LONG`` (the
fewest samples whose conv0 length exceeds 8192 frames: the 8192-frame chunk fold with a one-frame second chunk; for ``LONG_KINDS``),
and ``RAGGED_N``: one length per kind between 400 samples (T = 1, ``silence``) and ``N_SHORT``, all different, none a multiple of
320, odd and even conv0 lengths."""
from collections import OrderedDict

import torch

import degrade_ref
import ref64
from nomad_amd.weights import num_frames

SEED = 17
NAMES = ["silence", "constant", "dc_offset", "faint", "impulse", "square", "full_scale", "int16", "hard_clipped", "noisy_m20db",
         "half_silent"]
QUIET = ["silence", "constant", "dc_offset", "faint", "impulse"]      # rstd amplifies these: the large parameter gradients
LOUD = [k for k in NAMES if k not in QUIET]
LONG_KINDS = ["dc_offset", "constant", "half_silent"]


def conv0_frames(n: int) -> int:
    return (n - 10) // 5 + 1


N_SHORT = ref64.n_for(65)
N_LONG = 5 * 8192 + 10
assert N_SHORT == 20880 and conv0_frames(N_SHORT) == 4175
assert conv0_frames(N_LONG) == 8193 and conv0_frames(N_LONG - 1) == 8192

# frames and samples on top of ref64.n_for(T) per kind (fewer than 320, so T stays)
_RAGGED = {"silence": (1, 0), "constant": (2, 37), "dc_offset": (64, 111), "faint": (35, 5), "impulse": (17, 150), "square": (50, 83),
           "full_scale": (33, 163), "int16": (60, 251), "hard_clipped": (41, 301), "noisy_m20db": (57, 12), "half_silent": (65, 0)}
RAGGED_N = OrderedDict((k, ref64.n_for(_RAGGED[k][0]) + _RAGGED[k][1]) for k in NAMES)
assert all(num_frames(RAGGED_N[k]) == _RAGGED[k][0] and RAGGED_N[k] % 320 for k in NAMES)
assert len(set(RAGGED_N.values())) == len(NAMES) and min(RAGGED_N.values()) == RAGGED_N["silence"] == 400
assert max(RAGGED_N.values()) == RAGGED_N["half_silent"] == N_SHORT
assert {conv0_frames(n) % 2 for n in RAGGED_N.values()} == {0, 1}


def kinds(n: int, seed: int = SEED) -> "OrderedDict[str, torch.Tensor]":
    """{name: (n,) fp32 waveform} in the order of ``NAMES``."""
    g = torch.Generator().manual_seed(seed)
    base = (0.1 * torch.randn(n, generator=g)).clamp(-1, 1)
    t = torch.arange(n, dtype=torch.float32)
    out = OrderedDict()
    out["silence"] = torch.zeros(n)
    out["constant"] = torch.full((n,), 0.5)
    out["dc_offset"] = 0.5 + 1e-3 * torch.randn(n, generator=g)
    out["faint"] = 1e-4 * torch.randn(n, generator=g)
    out["impulse"] = torch.zeros(n).index_fill_(0, torch.tensor([n // 2]), 1.0)
    out["square"] = torch.sign(torch.sin(2 * torch.pi * 220.0 * t / 16000.0))
    out["full_scale"] = torch.randn(n, generator=g).clamp(-1, 1)
    out["int16"] = torch.round(base * 32768) / 32768
    out["hard_clipped"] = torch.from_numpy(degrade_ref.clip(base.numpy(), [40.0])[0][0].copy())
    out["noisy_m20db"] = torch.from_numpy(degrade_ref.noise(base.numpy(), torch.randn(n, generator=g).numpy(), [-20.0])[0][0].copy())
    half = base.clone()
    half[n // 2:] = 0.0
    out["half_silent"] = half
    assert list(out) == NAMES and all(v.dtype == torch.float32 and v.shape == (n,) for v in out.values())
    return out


def batch(n: int = N_SHORT, names=None, seed: int = SEED):
    """-> (names, (B, n) fp32): the kinds (all, or ``names``) of n samples as one batch."""
    names = list(names) if names is not None else list(NAMES)
    k = kinds(n, seed)
    return names, torch.stack([k[name] for name in names])


def ragged(seed: int = SEED):
    """-> (names, [1-D fp32 clips]): every kind at its own length (``RAGGED_N``), from a generator of its own."""
    return list(NAMES), [kinds(RAGGED_N[name], seed + 1 + i)[name] for i, name in enumerate(NAMES)]


def triplet_group(names, n: int = N_SHORT, seed: int = SEED):
    """Anchors: the kinds of ``names``; positives: the same plus 1e-3 randn; negatives: the anchors rotated by one."""
    _, A = batch(n, names, seed)
    g = torch.Generator().manual_seed(seed + 1000 + len(names))
    P = A + 1e-3 * torch.randn(A.shape, generator=g)
    return A, P, torch.roll(A, 1, 0)


def conv0_fold_restated(sd, wav: torch.Tensor) -> torch.Tensor:
    """The engine's conv0 + GroupNorm + GELU formulation restated on the CPU (nomad_amd/csrc/frontend.hip.h): float64 one-pass
    statistics from the waveform's 10 x 10 frame autocorrelation (var = s2 / L0 - mean^2, clamped at 0), fp32 scale = rstd gamma and
    shift = beta - mean rstd gamma, fp32 y = sum_j w_j x_j, z = y scale + shift, GELU.  wav (n,) fp32 -> (L0, 512) fp32."""
    P = "ssl_model.feature_extractor.conv_layers.0."
    w, gamma, beta = sd[P + "0.weight"].reshape(512, 10), sd[P + "2.weight"], sd[P + "2.bias"]
    X = wav.unfold(0, 10, 5)                                    # (L0, 10)
    L0 = X.shape[0]
    Xd, wd = X.double(), w.double()
    S, R = Xd.sum(0), Xd.T @ Xd
    mean = (wd @ S) / L0
    var = (torch.einsum("cj,jk,ck->c", wd, R, wd) / L0 - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = (rstd * gamma.double()).float()
    shift = (beta.double() - mean * rstd * gamma.double()).float()
    y = X.float() @ w.float().T
    return torch.nn.functional.gelu(y * scale + shift)


def conv0_stats64(sd, wav: torch.Tensor):
    """-> (mean (512,), var (512,)) of conv0's output over time, two-pass in float64."""
    w = sd["ssl_model.feature_extractor.conv_layers.0.0.weight"].reshape(512, 10).double()
    y = wav.double().unfold(0, 10, 5) @ w.T
    return y.mean(0), y.var(0, unbiased=False)
