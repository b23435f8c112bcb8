"""CPU: the gradient conventions of include/nomad_hip.h ("NSIM as a loss") as ``nsim_grad_ref`` restates them - the forward agrees with
``nsim_ref.nsim``, the gradient with directional central differences on cuts that reach every branch of the conventions - and the
argument checks of ``Nomad.nsim_loss``, which raise before any engine call.

The cuts are samples 8000 .. 12800 of tests/golden/wavs/nmr-data/FI53_04.wav (``nsim_grad_ref.cases``, noise = ``pcm_noise(4800, 3)``):
  a  noise at 10 dB                                                            tolerance 1e-5
  b  clip factor 20                                                            1e-5
  c  noise at 5 dB with samples 1600 .. 3400 zeroed (47 degraded cells on the absolute floor, 2 cells with zero variance)   1e-5
  d  the cut x 1000 as the clean row, noise at 15 dB with samples 0 .. 1500 scaled by 1e-4 as the degraded one
     (degraded cells on the per-frame floor)                                   1e-4
  e  case d with the roles swapped (clean cells on a floor set by a degraded peak, 12 frames with the peak in the degraded row)   1e-3
Central differences on float64 copies, step 1e-5 x the row's peak, one unit random direction.  Each case asserts its counters, so it
cannot pass without reaching its branch.  Measured here: forward distance <= 7e-15; relative disagreement a 1.2e-7, b 1.3e-6,
c 1.2e-7, d 4.5e-8, e 6.2e-8 (the step's own rounding: the loss moves by 1e-8 over it); counters c 47 floored / 2 zero-variance cells,
d 64 degraded cells on the per-frame floor, e 64 clean cells on a floor set by a degraded peak in 12 frames; identical rows
|gradient| 1.9e-15."""
import os

import numpy as np
import pytest
import torch

import nsim_grad_ref as GR
import nsim_ref as N
from conftest import ROOT
from nomad_amd import wavio
from nomad_amd.nomad import Nomad

TOL = {"a": 1e-5, "b": 1e-5, "c": 1e-5, "d": 1e-4, "e": 1e-3}


@pytest.fixture(scope="module")
def cuts():
    x, fs = wavio.read_wav(os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data", "FI53_04.wav"))
    assert fs == 16000
    return GR.cases(np.asarray(x, dtype=np.float32).reshape(-1))


def _loss(clean, est64):
    with torch.no_grad():
        return 1.0 - float(GR.nsim(torch.from_numpy(clean).double(), torch.from_numpy(est64))[0])


@pytest.mark.parametrize("name", sorted(TOL))
def test_gradient_agrees_with_central_differences(cuts, name):
    clean, est = cuts[name]
    score, g, counters = GR.loss_grad(clean, est)
    want = N.nsim(clean, est)[0]
    print(f"case {name}: NSIM {score!r}, nsim_ref {want!r}, counters {counters}")
    assert abs(score - want) <= 1e-13, (score, want)
    assert np.isfinite(g).all()
    u = np.random.RandomState(3).randn(est.shape[0])
    u /= np.linalg.norm(u)
    h = 1e-5 * float(np.abs(est).max())
    e64 = est.astype(np.float64)
    fd = (_loss(clean, e64 + h * u) - _loss(clean, e64 - h * u)) / (2.0 * h)
    an = float(g @ u)
    rel = abs(fd - an) / abs(fd)
    print(f"case {name}: central difference {fd!r}, gradient {an!r}, relative disagreement {rel:.3g} (tolerance {TOL[name]:g})")
    if name == "c":
        assert counters["abs_floor_deg"] >= 1 and counters["zero_var"] >= 1, counters
    if name == "d":
        assert counters["frame_floor_deg"] >= 1, counters
    if name == "e":
        assert counters["frame_floor_clean_deg_peak"] >= 1 and counters["deg_peak_frames"] >= 1 and np.abs(g).max() > 0.0, counters
    assert rel <= TOL[name], (fd, an, rel)


def test_identical_rows_give_one_and_no_gradient(cuts):
    x = cuts["a"][0]
    score, g, _ = GR.loss_grad(x, x)
    print(f"identical rows: NSIM {score!r}, largest |gradient| {np.abs(g).max():.3g}")
    assert score == 1.0
    assert np.abs(g).max() <= 1e-12


def test_silent_frames_keep_the_gradient_finite(cuts):
    clean, est = cuts["c"]
    est = est.copy()
    est[:1280] = 0.0                                       # frame 0 is digital silence
    score, g, counters = GR.loss_grad(clean, est)
    assert np.isfinite(score) and np.isfinite(g).all() and counters["abs_floor_deg"] >= 21


class _NoEngine:
    """Any use of the engine is a failure: the checks come first."""
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name}) before the arguments were checked")


def test_nsim_loss_checks_its_arguments_before_any_engine_call():
    n = Nomad.__new__(Nomad)
    n.engine, n.precision, n.group = _NoEngine(), "fp32", None
    est, clean = torch.zeros(2, 1, 4000), torch.zeros(2, 1, 4000)
    with pytest.raises(ValueError, match="reduction"):
        n.nsim_loss(est, clean, reduction="sum")
    with pytest.raises(ValueError, match=r"estimate must be \(B,1,N\) or \(B,N\)"):
        n.nsim_loss(torch.zeros(4000), clean)
    with pytest.raises(ValueError, match=r"estimate must be \(B,1,N\) or \(B,N\)"):
        n.nsim_loss(torch.zeros(2, 2, 4000), torch.zeros(2, 2, 4000))
    with pytest.raises(ValueError, match="clean must have estimate's shape"):
        n.nsim_loss(est, torch.zeros(2, 1, 4001))
    with pytest.raises(ValueError, match="clean must not require a gradient"):
        n.nsim_loss(est, clean.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="intensity_range"):
        n.nsim_loss(est, clean, intensity_range=0.0)
    with pytest.raises(ValueError, match="shorter than one frame"):
        n.nsim_loss(torch.zeros(2, 1279), torch.zeros(2, 1279))
    with pytest.raises(ValueError, match="shorter than one frame"):
        n.nsim_loss(est, clean, lengths=[4000, 1279])
    with pytest.raises(ValueError, match="lengths"):
        n.nsim_loss(est, clean, lengths=[4000])
    with pytest.raises(ValueError, match="outside"):
        n.nsim_loss(est, clean, lengths=[4000, 4001])
