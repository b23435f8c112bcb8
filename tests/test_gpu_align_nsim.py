"""GPU: NSIM of rows that are NOT sample-aligned with their clean clips - ``Nomad.nsim(max_delay_s=...)``, ``Nomad.align``,
``Nomad.nsim_files`` and the CLI's ``--nsim-pairs``.

* clean clips of 4000 and 9001 samples, ``degrade(noise)`` at 20 and 5 dB SNR; every row is then delayed on the host by -300, 0, 37
  and 1105 samples and lengthened (8 rows per clip).  Through ``nsim(max_delay_s=0.1)`` the delays come back exactly and the NSIM
  has the bits of ``nsim`` on rows aligned on the host; the plain ``nsim`` of the shifted rows - what a caller got before - is lower.
* ``nsim(max_delay_s=None)`` has the plain call's bits.
* ``nsim_files`` and the CLI over a temporary folder of wav files written from the golden clips with known delays: the table's
  columns and delays, the NSIM of the tensor path, NaN for a clean file under 80 ms."""
import os
import struct

import numpy as np
import pandas as pd
import pytest
import torch

import align_ref
import nsim_ref as N
from conftest import ROOT

pytestmark = pytest.mark.gpu

LENS = [4000, 9001]
SNR = [20.0, 5.0]
DELAYS = [-300, 0, 37, 1105]


def _speechlike(n, seed):
    rng = np.random.RandomState(seed)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0 + seed)
    return (np.round(np.clip(0.2 * env * rng.randn(n), -1, 1) * 32767) / 32768.0).astype(np.float32)


def _write_wav(path, x, sr=16000):
    pcm = np.round(np.clip(x, -1, 1) * 32768.0).clip(-32768, 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" +
                struct.pack("<I", len(pcm)) + pcm)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def nomad(engine):
    from nomad_amd.nomad import Nomad
    return Nomad.from_engine(engine)


def test_delayed_rows_get_the_nsim_of_the_aligned_rows(nomad):
    clean = torch.zeros(2, max(LENS))
    for b, n in enumerate(LENS):
        clean[b, :n] = torch.from_numpy(_speechlike(n, 3 + b))
    noise = torch.from_numpy(N.pcm_noise(5000, 9, 0.2))
    rows, lens_rep = nomad.degrade(clean, "noise", SNR, noise=noise, lengths=LENS)
    host = rows.cpu().numpy()
    G = len(SNR) * len(DELAYS)
    width = max(LENS) + 1400
    shifted, dlens = torch.zeros(2 * G, width), []
    aligned, cut = torch.zeros(2 * G, 9004), torch.zeros(2 * G, 9004)      # packed rows: a stride that is a multiple of 4
    for b, n in enumerate(LENS):
        for s in range(len(SNR)):
            for k, d in enumerate(DELAYS):
                r = b * G + s * len(DELAYS) + k
                m = n + 1200 + 13 * k
                y = align_ref.shift(host[b * len(SNR) + s, :n], -d, m)            # the row late by d samples, lengthened
                shifted[r, :m] = torch.from_numpy(y)
                dlens.append(m)
                aligned[r, :n] = torch.from_numpy(align_ref.shift(y, d, n))       # aligned on the host
                cut[r, :n] = torch.from_numpy(y[:n])                              # what a caller had before: the row as it came, cut
    lens8 = [n for n in LENS for _ in range(G)]
    score, delay = nomad.nsim(shifted, clean, lengths=LENS, max_delay_s=0.1, degraded_lengths=dlens)
    assert score.shape == (2, G) and score.dtype == torch.float64 and delay.shape == (2, G) and delay.dtype == torch.int32
    assert delay.cpu().tolist() == [DELAYS * len(SNR)] * 2, "the delays are recovered exactly"
    want = nomad.nsim((aligned.to(score.device), lens8), clean, lengths=LENS)
    assert np.array_equal(_bits(score), _bits(want)), "the NSIM of the rows aligned on the host, bit for bit"
    plain = nomad.nsim((cut.to(score.device), lens8), clean, lengths=LENS).cpu().numpy()
    got = score.cpu().numpy()
    print("aligned", got.round(4).tolist(), "unaligned", plain.round(4).tolist())
    for r in range(2 * G):
        b, k = divmod(r, G)
        if DELAYS[k % len(DELAYS)] == 0:
            assert plain[b, k] == got[b, k]
        else:
            assert plain[b, k] < got[b, k], "the unaligned NSIM of a shifted row is lower: what was silently wrong before"
    # the packed form, with bands, and Nomad.align feeding nsim by hand
    packed = nomad.engine._pack([shifted[r, :m] for r, m in enumerate(dlens)])
    score2, bands2, delay2 = nomad.nsim(packed, clean, lengths=LENS, max_delay_s=0.1, bands=True)
    assert np.array_equal(_bits(score2), _bits(score)) and torch.equal(delay2, delay) and bands2.shape == (2, G, 21)
    (moved, mlens), delay3, peak3 = nomad.align(shifted, clean, lengths=LENS, degraded_lengths=dlens, max_delay_s=0.1)
    assert mlens == lens8 and torch.equal(delay3.view(2, G), delay) and bool(torch.isfinite(peak3).all())
    for r in range(2 * G):
        assert torch.equal(moved[r, :lens8[r]].cpu(), aligned[r, :lens8[r]]) and not moved[r, lens8[r]:].any()
    assert np.array_equal(_bits(nomad.nsim((moved, mlens), clean, lengths=LENS)), _bits(score))


def test_without_max_delay_the_call_is_the_plain_one(nomad):
    clean = torch.zeros(2, max(LENS))
    for b, n in enumerate(LENS):
        clean[b, :n] = torch.from_numpy(_speechlike(n, 5 + b))
    rows, lens_rep = nomad.degrade(clean, "clip", [10.0, 40.0], lengths=LENS)
    a = nomad.nsim((rows, lens_rep), clean, lengths=LENS)
    b_ = nomad.nsim((rows, lens_rep), clean, lengths=LENS, max_delay_s=None)
    spec_ref, frames = nomad.engine.gammatone(packed=nomad.engine._rows(clean.to(rows.device), LENS, None))
    spec_deg, _ = nomad.engine.gammatone(packed=(rows, lens_rep))
    direct = nomad.engine.nsim_of_spectrograms(spec_ref, spec_deg, frames, 2, want_bands=False)[0]
    assert torch.is_tensor(a) and np.array_equal(_bits(a), _bits(b_)) and np.array_equal(_bits(a), _bits(direct))
    # aligned rows found at delay 0 keep the plain value too
    c, delay = nomad.nsim((rows, lens_rep), clean, lengths=LENS, max_delay_s=0.1)
    assert not delay.any() and np.array_equal(_bits(c), _bits(a))


FILE_DELAYS = [-300, 0, 37, 1105]


@pytest.fixture(scope="module")
def pair_files(tmp_path_factory, nomad):
    """Four golden clips (their first 2 s) as ref_k.wav, each late by a known delay, lengthened and with a little noise as deg_k.wav;
    a fifth pair whose clean file is under 80 ms."""
    folder = tmp_path_factory.mktemp("pairs")
    src = os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data")
    refs, degs = [], []
    for k, name in enumerate(sorted(os.listdir(src))):
        x = nomad.load_processing(os.path.join(src, name)).reshape(-1).numpy()[:32000 - 700 * k]
        y = align_ref.shift(x, -FILE_DELAYS[k], x.shape[0] + 1300 + k) + 0.002 * N.pcm_noise(x.shape[0] + 1300 + k, 40 + k, 0.25)
        refs.append(str(folder / f"ref_{k}.wav"))
        degs.append(str(folder / f"deg_{k}.wav"))
        _write_wav(refs[-1], x)
        _write_wav(degs[-1], y)
    refs.append(str(folder / "ref_short.wav"))
    degs.append(str(folder / "deg_short.wav"))
    _write_wav(refs[-1], _speechlike(1000, 1))
    _write_wav(degs[-1], align_ref.shift(_speechlike(1000, 1), -5, 1100))
    csv = str(folder / "degraded_data_visqol_format.csv")
    pd.DataFrame({"filepath_ref": refs, "filepath_deg": degs}).to_csv(csv, index=False)
    return refs, degs, csv


def test_nsim_files_is_the_tensor_path_per_pair(nomad, pair_files, tmp_path):
    refs, degs, csv = pair_files
    table = nomad.nsim_files(csv, max_delay_s=0.1, results_path=str(tmp_path))
    assert list(table.columns) == ["filepath_ref", "filepath_deg", "delay_samples", "delay_s", "NSIM"]
    assert table["filepath_ref"].tolist() == refs and table["filepath_deg"].tolist() == degs
    assert table["delay_samples"].tolist() == FILE_DELAYS + [5]
    assert np.array_equal(table["delay_s"].to_numpy(), np.asarray(FILE_DELAYS + [5]) / 16000.0)
    assert np.isnan(table["NSIM"].iloc[4]) and np.isfinite(table["NSIM"].iloc[:4]).all()
    for k in range(4):
        x, y = nomad.load_processing(refs[k]), nomad.load_processing(degs[k])
        score, delay = nomad.nsim(y, x, max_delay_s=0.1)
        assert int(delay) == FILE_DELAYS[k] and np.array_equal(_bits(score.reshape(-1)), _bits(table["NSIM"].to_numpy()[k:k + 1])), k
        assert 0.0 < float(score) <= 1.0
    written = pd.read_csv(tmp_path / "nsim_pairs.csv")
    assert list(written.columns) == list(table.columns) and written["delay_samples"].tolist() == FILE_DELAYS + [5]
    assert np.allclose(written["NSIM"].to_numpy()[:4], table["NSIM"].to_numpy()[:4], rtol=1e-12, atol=0) and np.isnan(written["NSIM"].iloc[4])
    # two lists of paths, one pair per batch: the same table
    again = nomad.nsim_files(degs, refs, max_delay_s=0.1, max_batch_samples=1)
    assert np.array_equal(again["delay_samples"].to_numpy(), table["delay_samples"].to_numpy())
    assert np.array_equal(_bits(again["NSIM"].to_numpy()), _bits(table["NSIM"].to_numpy()))


def test_cli_nsim_pairs_writes_the_table(nomad, pair_files, tmp_path, capsys):
    from nomad_amd import __main__ as cli
    refs, degs, csv = pair_files
    want = nomad.nsim_files(csv, max_delay_s=0.1)
    cli.main(["--nsim-pairs", csv, "--max-delay", "0.1", "--results_path", str(tmp_path), "--weights", "seeded"])
    assert "NSIM of the aligned pairs" in capsys.readouterr().out
    written = pd.read_csv(tmp_path / "nsim_pairs.csv")
    assert list(written.columns) == ["filepath_ref", "filepath_deg", "delay_samples", "delay_s", "NSIM"]
    assert written["filepath_deg"].tolist() == degs and written["delay_samples"].tolist() == want["delay_samples"].tolist()
    assert np.allclose(written["NSIM"].to_numpy()[:4], want["NSIM"].to_numpy()[:4], rtol=1e-12, atol=0) and np.isnan(written["NSIM"].iloc[4])
