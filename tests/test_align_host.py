"""CPU: the host side of the time alignment - tests/align_ref.py against scipy and hand-made tables, the argument checks of
``Nomad.align`` / ``Nomad.nsim(max_delay_s=)`` / ``Nomad.nsim_files`` that need no GPU, the pairs csv, the CLI's refusals."""
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import align_ref
from nomad_amd.nomad import Nomad, check_max_delay, pairs_from_csv


@pytest.mark.parametrize("n,m,D", [(1, 1, 0), (1, 5, 3), (7, 7, 0), (16, 11, 20), (33, 70, 5), (255, 292, 128), (257, 252, 300)])
def test_reference_correlation_is_scipys(n, m, D):
    from scipy.signal import correlate, correlation_lags
    rng = np.random.RandomState(n + m + D)
    x, y = rng.randint(-8, 9, size=n).astype(np.float64), rng.randint(-8, 9, size=m).astype(np.float64)
    full = correlate(y, x, mode="full", method="direct")          # full[k]: lag k - (n - 1) of y against x
    lags = correlation_lags(m, n, mode="full")
    want = np.zeros(2 * D + 1)
    for v, d in zip(full, lags):
        if -D <= d <= D:
            want[d + D] = v
    got = align_ref.corr(x, y, D)
    assert got.shape == (2 * D + 1,) and np.array_equal(got, want)
    mag = align_ref.magnitude(x, y, D)
    assert np.array_equal(mag, align_ref.corr(np.abs(x), np.abs(y), D)) and (mag >= np.abs(got)).all()
    # the definition itself, term by term
    for d in (-D, -1 if D else 0, 0, D):
        s = sum(x[i] * y[i + d] for i in range(n) if 0 <= i + d < m)
        assert got[d + D] == s


def test_selection_rule_on_hand_made_tables():
    nan = float("nan")
    assert align_ref.select([0.0, 1.0, 5.0, 1.0, 0.0], 2) == (0, 5.0)
    assert align_ref.select([9.0, 1.0, 5.0, 1.0, 0.0], 2) == (-2, 9.0)
    assert align_ref.select([-3.0, -1.0, -2.0], 1) == (0, -1.0), "the sign counts: the largest value, not the largest magnitude"
    assert align_ref.select([-9.0, -1.0, -2.0], 1) == (0, -1.0)
    assert align_ref.select([4.0, 1.0, 4.0], 1) == (1, 4.0), "equal |d|: the non-negative lag"
    assert align_ref.select([4.0, 4.0, 1.0, 0.0, 4.0], 2) == (-1, 4.0), "ties go to the smaller |d|"
    assert align_ref.select([4.0, 0.0, 1.0, 4.0, 4.0], 2) == (1, 4.0)
    assert align_ref.select([0.0] * 7, 3) == (0, 0.0), "a silent row ties everywhere"
    assert align_ref.select([7.0], 0) == (0, 7.0)
    d, p = align_ref.select([1.0, nan, 9.0], 1)
    assert d == 0 and np.isnan(p)
    d, p = align_ref.select([nan] * 3, 1)
    assert d == 0 and np.isnan(p)
    assert align_ref.select([1.0, float("inf"), 2.0, float("inf"), 0.0], 2) == (1, float("inf"))


def test_reference_shift():
    y = np.arange(1, 8, dtype=np.float32)
    assert align_ref.shift(y, 0, 5).tolist() == [1, 2, 3, 4, 5]
    assert align_ref.shift(y, 2, 5).tolist() == [3, 4, 5, 6, 7]
    assert align_ref.shift(y, 4, 5, stride=8).tolist() == [5, 6, 7, 0, 0, 0, 0, 0]
    assert align_ref.shift(y, -2, 5).tolist() == [0, 0, 1, 2, 3]
    assert align_ref.shift(y, -9, 5).tolist() == [0] * 5 and align_ref.shift(y, 7, 5).tolist() == [0] * 5
    assert align_ref.shift(y, 0, 9).tolist() == [1, 2, 3, 4, 5, 6, 7, 0, 0]


def test_max_delay_in_seconds():
    assert check_max_delay(0) == 0 and check_max_delay(0.25) == 4000 and check_max_delay(1.024) == 16384 and check_max_delay(0.1) == 1600
    for bad in (-0.001, 1.0241, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="max_delay_s"):
            check_max_delay(bad)


class _NoEngine:
    device = "cpu"

    def __getattr__(self, name):
        pytest.fail(f"an argument error reached the engine ({name})")


def _nomad():
    n = Nomad.__new__(Nomad)            # no GPU: only the host side is under test
    n.engine, n.precision, n.group = _NoEngine(), "fp32", None
    return n


@pytest.mark.parametrize("call", ["align", "nsim"])
def test_align_and_aligned_nsim_refusals(call):
    n = _nomad()
    clean, deg = torch.zeros(2, 8000), torch.zeros(4, 8100)

    def run(d, c, **kw):
        kw.setdefault("max_delay_s", 0.1)
        return n.align(d, c, **kw) if call == "align" else n.nsim(d, c, **kw)

    with pytest.raises(ValueError, match="produces no gradient"):
        run(deg, clean.clone().requires_grad_())
    with pytest.raises(ValueError, match="produces no gradient"):
        run(deg.clone().requires_grad_(), clean)
    with pytest.raises(ValueError, match="produces no gradient"):
        run((deg.clone().requires_grad_(), [8100] * 4), clean)
    with pytest.raises(ValueError, match="max_delay_s"):
        run(deg, clean, max_delay_s=2.0)
    with pytest.raises(ValueError, match="max_delay_s"):
        run(deg, clean, max_delay_s=-1.0)
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        run(deg, torch.zeros(8000))
    with pytest.raises(ValueError, match="G rows per clean clip"):
        run(torch.zeros(3, 8100), clean)
    with pytest.raises(ValueError, match="G rows per clean clip"):
        run(torch.zeros(130, 10), clean)
    with pytest.raises(ValueError, match="degraded_lengths go with a tensor"):
        run((deg, [8100] * 4), clean, degraded_lengths=[8100] * 4)
    with pytest.raises(ValueError, match="one entry per"):
        run(deg, clean, degraded_lengths=[8100] * 3)
    with pytest.raises(ValueError, match="one entry per"):
        run((deg, [8100] * 3), clean)
    with pytest.raises(ValueError, match="1 .. the width"):
        run(deg, clean, degraded_lengths=[8100, 8101, 5, 5])
    with pytest.raises(ValueError, match="1 .. the width"):
        run(deg, clean, lengths=[0, 8000])
    with pytest.raises(ValueError, match="packed"):
        run((deg, [8100] * 4, None), clean)


def test_plain_nsim_refuses_degraded_lengths():
    n = _nomad()
    with pytest.raises(ValueError, match="degraded_lengths go with max_delay_s"):
        n.nsim(torch.zeros(2, 8000), torch.zeros(2, 8000), degraded_lengths=[8000, 8000])


def test_pairs_csv(tmp_path):
    table = pd.DataFrame({"filepath_deg": ["d0.wav", "d1.wav", "d2.wav"], "extra": [1, 2, 3], "filepath_ref": ["r0.wav", "r1.wav", "r0.wav"]})
    path = tmp_path / "degraded_data_visqol_format.csv"
    table.to_csv(path, index=False)
    for source in (str(path), path, table):
        refs, degs = pairs_from_csv(source)
        assert refs == ["r0.wav", "r1.wav", "r0.wav"] and degs == ["d0.wav", "d1.wav", "d2.wav"]
    with pytest.raises(ValueError, match="filepath_ref"):
        pairs_from_csv(table.drop(columns=["filepath_ref"]))
    with pytest.raises(ValueError, match="filepath_deg"):
        pairs_from_csv(table.rename(columns={"filepath_deg": "filename"}))
    with pytest.raises(ValueError, match="no rows"):
        pairs_from_csv(table.iloc[:0])
    with pytest.raises(ValueError, match="does not exist"):
        pairs_from_csv(str(tmp_path / "missing.csv"))
    holed = table.copy()
    holed.loc[1, "filepath_deg"] = None
    with pytest.raises(ValueError, match="empty"):
        pairs_from_csv(holed)
    with pytest.raises(ValueError, match="csv path or a DataFrame"):
        pairs_from_csv(["a.wav"])


def test_nsim_files_refusals(tmp_path):
    n = _nomad()
    with pytest.raises(ValueError, match="as many clean files"):
        n.nsim_files(["a.wav", "b.wav"], ["c.wav"])
    with pytest.raises(ValueError, match="as many clean files"):
        n.nsim_files([], [])
    with pytest.raises(ValueError, match="two lists of paths"):
        n.nsim_files("a.wav", ["c.wav"])
    with pytest.raises(ValueError, match="max_delay_s"):
        n.nsim_files(["a.wav"], ["c.wav"], max_delay_s=3.0)
    with pytest.raises(ValueError, match="does not exist"):
        n.nsim_files(str(tmp_path / "missing.csv"))


@pytest.mark.parametrize("extra,word", [(["--max-delay", "0.1"], "--nsim-pairs"), (["--nsim-pairs", "p.csv", "--max-delay", "2"], "--max-delay"),
                                        (["--nsim-pairs", "p.csv", "--max-delay", "nan"], "--max-delay"),
                                        (["--nsim-pairs", "p.csv", "--sweep", "--clip", "5"], "--nsim-pairs"),
                                        (["--nsim-pairs", "p.csv", "--window", "1"], "--nsim-pairs")])
def test_cli_refusals(extra, word, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_hands_the_csv_to_nsim_files(monkeypatch, capsys, tmp_path):
    from nomad_amd import __main__ as cli
    seen = {}

    class Fake:
        def __init__(self, **kw):
            pass

        def nsim_files(self, pairs, max_delay_s, results_path):
            seen.update(pairs=pairs, max_delay_s=max_delay_s, results_path=results_path)
            return pd.DataFrame({"filepath_ref": ["r"], "filepath_deg": ["d"], "delay_samples": [3], "delay_s": [3 / 16000], "NSIM": [0.5]})

    monkeypatch.setattr(cli, "Nomad", Fake)
    cli.main(["--nsim-pairs", "pairs.csv", "--max-delay", "0.05", "--results_path", str(tmp_path)])
    assert seen == {"pairs": "pairs.csv", "max_delay_s": 0.05, "results_path": str(tmp_path)}
    cli.main(["--nsim-pairs", "pairs.csv"])
    assert seen["max_delay_s"] == 0.25 and seen["results_path"] is None
    assert "delay_samples" in capsys.readouterr().out
