"""CPU: properties of the restatement ``nsim_ref`` of the gammatone-spectrogram NSIM (include/nomad_hip.h states the measure; it
is modelled on ViSQOL's speech mode from memory and was never compared with the ViSQOL binary, so what is held here are
properties, not ViSQOL's numbers).  Subject: tests/golden/wavs/nmr-data/FI53_04.wav (30 671 samples at 16 kHz, 92 frames) with
``RandomState(0).randn`` noise mixed by the reference's formula, and clipped at the reference's percentiles.

Seen while drafting (float64 prototype): NSIM at 40 .. -5 dB SNR in steps of 5: 0.999998, 0.99998, 0.99968, 0.9957, 0.9768, 0.9292,
0.8221, 0.6328, 0.4272, 0.2582; at clip factors 1, 5, 10, 20, 40, 60, 80: 0.9918, 0.9318, 0.8841, 0.8262, 0.7324, 0.5812, 0.1600.  The
tests assert the two orderings, not the digits."""
import os

import numpy as np
import pytest

import nsim_ref as N
from conftest import ROOT
from nomad_amd import wavio

SNRS = [40, 35, 30, 25, 20, 15, 10, 5, 0, -5]
CLIPS = [1, 5, 10, 20, 40, 60, 80]


@pytest.fixture(scope="module")
def subject():
    x, fs = wavio.read_wav(os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data", "FI53_04.wav"))
    assert fs == 16000
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    assert x.shape[0] == 30671 and N.frames_of(x.shape[0]) == 92
    return x, N.spectrogram(x).astype(np.float64)


def test_band_centres_and_unit_response_at_the_centre():
    cf = N.centres()
    assert cf.shape == (21,) and (np.diff(cf) > 0).all(), cf
    assert abs(cf[0] - 50.0) < 1e-9 and cf[-1] < 8000.0, cf
    for fs in (16000, 22050, 48000):
        resp = N.response_at_centre(fs)
        assert np.abs(resp - 1.0).max() <= 1e-12, (fs, resp)


def test_frame_count():
    assert [N.frames_of(n) for n in (1279, 1280, 1599, 1600, 1920, 30671)] == [0, 1, 1, 2, 3, 92]
    assert N.frames_of(3839, 48000) == 0 and N.frames_of(3840, 48000) == 1 and N.frames_of(33333, 48000) == 31


def test_a_spectrogram_with_itself_is_one(subject):
    _, S = subject
    score, bands, m = N.nsim_map(S, S)
    assert abs(score - 1.0) <= 1e-12 and np.abs(bands - 1.0).max() <= 1e-12 and m.shape == (92, 21)


def test_nsim_falls_strictly_with_the_snr(subject):
    x, S = subject
    noise = np.random.RandomState(0).randn(x.shape[0])
    got = [float(N.nsim_map(S, N.spectrogram(N.add_noise(x, noise, snr)).astype(np.float64))[0]) for snr in SNRS]
    print("NSIM at SNR", dict(zip(SNRS, got)))
    assert all(a > b for a, b in zip(got, got[1:])), got
    assert got[0] < 1.0 and got[-1] > 0.0, got


def test_nsim_falls_strictly_with_the_clip_factor(subject):
    x, S = subject
    got = [float(N.nsim_map(S, N.spectrogram(N.clip(x, cf)).astype(np.float64))[0]) for cf in CLIPS]
    print("NSIM at clip factor", dict(zip(CLIPS, got)))
    assert all(a > b for a, b in zip(got, got[1:])), got
    assert got[0] < 1.0, got


def test_silence_zeros_and_non_finite_samples():
    zeros = np.zeros(1600, dtype=np.float32)
    S0 = N.spectrogram(zeros)
    assert S0.shape == (2, 21) and not S0.any()
    score, bands, _ = N.nsim_map(S0.astype(np.float64), S0.astype(np.float64))
    assert score == 1.0 and (bands == 1.0).all(), "a silent pair gives exactly 1"
    x = N.pcm_noise(1920, 3)
    bad = x.copy()
    bad[1500] = np.nan            # frames 1 (320 .. 1599) and 2 (640 .. 1919) hold it, frame 0 (0 .. 1279) does not
    S, Sb = N.spectrogram(x), N.spectrogram(bad)
    assert np.isnan(Sb[1:]).all() and np.array_equal(Sb[0], S[0])
    score, bands, _ = N.nsim_map(S.astype(np.float64), Sb.astype(np.float64))
    assert np.isnan(score) and np.isnan(bands).all()


# ---- the CLI's --nsim ----------------------------------------------------------------------------------------------------------
def _fake_cli(monkeypatch, tmp_path, extra):
    import sys

    import pandas as pd
    from nomad_amd import __main__ as cli
    nmr, deg, out = tmp_path / "nmr", tmp_path / "clean", tmp_path / "out"
    for d in (nmr, deg, out):
        d.mkdir(exist_ok=True)
    seen = {}

    class _Fake:
        def __init__(self, **kw):
            pass

        def get_embeddings(self, path):
            return pd.concat([pd.DataFrame({"filename": ["r0", "r1"]}), pd.DataFrame(np.ones((2, 256), dtype=np.float32))], axis=1)

        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, k=None, **kw):
            seen.update(kw)
            res = dict(table=pd.DataFrame({"Condition": [40.0, 5.0], "Distance": [0.4, 0.3]}), SRCC=1.0)
            if kw.get("nsim"):      # two clips at two levels, rows b G + g
                res.update(nsim=np.array([0.9, 0.5, 0.8, 0.3]), conditions=np.array([5.0, 40.0, 5.0, 40.0]))
            return {"CLIP": res}

    monkeypatch.setattr(cli, "Nomad", _Fake)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--mode", "dir", "--nmr", str(nmr), "--deg", str(deg), "--results_path", str(out),
                                      "--sweep", "--clip", "5,40"] + extra)
    cli.main()
    return seen, open(out / "nomad_intensity.csv").read()


def test_cli_nsim_adds_one_column_and_without_it_the_csv_is_unchanged(tmp_path, monkeypatch):
    seen, plain = _fake_cli(monkeypatch, tmp_path, [])
    assert seen == {} and plain.splitlines() == ["Degradation,Condition,NOMAD", "CLIP,5.0,0.3", "CLIP,40.0,0.4"]
    seen, with_nsim = _fake_cli(monkeypatch, tmp_path, ["--nsim"])
    assert seen == {"nsim": True}
    lines = with_nsim.splitlines()
    assert lines[0] == "Degradation,Condition,NOMAD,NSIM" and [l.rsplit(",", 1)[0] for l in lines] == plain.splitlines()
    assert [round(float(l.rsplit(",", 1)[1]), 12) for l in lines[1:]] == [0.85, 0.4], "the mean NSIM per level, in the table's order"


def test_cli_refuses_nsim_without_sweep(monkeypatch, capsys):
    import sys

    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b", "--nsim"])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and "--nsim goes with --sweep" in capsys.readouterr().err
