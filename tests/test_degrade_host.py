"""CPU: the host side of the on-device degradations - ``degrade_ref`` against numpy, the three exports, and the argument handling
of ``Nomad.degrade`` / ``Nomad.intensity_sweep`` / ``Training.eval_degradation_intensity`` / the CLI's ``--sweep`` against recording
fake engines (the kernels themselves: tests/test_gpu_degrade.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import degrade_ref
from knn_ref import knn_ref
from nomad_amd import train as T
from nomad_amd.nomad import Nomad


# ---- degrade_ref against numpy ---------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 255, 256, 257, 1025, 4099, 16000]
FACTORS = [0, 0.5, 2, 5, 11, 25, 40, 62, 99, 100]


def _inputs(n, seed):
    r = np.random.RandomState(seed)
    return {"pcm": (r.randint(-32768, 32768, size=n) / 32768.0).astype(np.float32),
            "gauss": (0.1 * r.randn(n)).astype(np.float32),
            "const": np.full(n, -0.375, dtype=np.float32),
            "seven": r.choice(np.linspace(-0.75, 0.75, 7).astype(np.float32), size=n).astype(np.float32)}


@pytest.mark.parametrize("n", LENGTHS)
def test_reference_thresholds_are_numpy_percentiles(n):
    """``np.percentile``'s linear rule interpolates as a + (b - a) t below t = 0.5 and as b - (b - a) (1 - t) above: the same
    order statistics and the same t, one rounding apart - 1e-14 absolute on samples within [-1, 1].  A clipped float32 sample then
    differs by at most one float32 rounding of a threshold: 2^-23 on values below 1."""
    for kind, x in _inputs(n, 1000 + n).items():
        rows, thr = degrade_ref.clip(x, FACTORS)
        xd = x.astype(np.float64)
        for g, cf in enumerate(FACTORS):
            vlo, vhi = np.percentile(xd, [cf / 2, 100 - cf / 2])
            assert abs(thr[g, 0] - vlo) <= 1e-14 and abs(thr[g, 1] - vhi) <= 1e-14, (kind, n, cf, thr[g], vlo, vhi)
            want = np.where(xd > vhi, np.float32(vhi), np.where(xd < vlo, np.float32(vlo), x))
            assert np.abs(rows[g].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23, (kind, n, cf)
        assert np.array_equal(rows[0], x), "level 0 clips nothing"
        assert (rows[-1] == np.float32(thr[-1, 0])).all() and thr[-1, 0] == thr[-1, 1], "level 100 is the median"


def test_reference_noise_is_the_stated_formula():
    r = np.random.RandomState(3)
    x = (0.2 * r.randn(1000)).astype(np.float32)
    s = (0.05 * r.randn(300)).astype(np.float32)
    rows, alpha, exact = degrade_ref.noise(x, s, [0, 15])
    tiled = np.tile(s.astype(np.float64), 4)[:1000]
    xp, sp = np.sqrt(np.mean(x.astype(np.float64) ** 2)), np.sqrt(np.mean(tiled ** 2))
    assert alpha[0] == (xp / 1.0) / sp and abs(alpha[1] - (xp / 10 ** 1.5) / sp) <= 1e-15 * alpha[1]
    assert np.array_equal(exact[1], x + alpha[1] * tiled) and rows.dtype == np.float32
    assert np.isnan(degrade_ref.noise(np.zeros(4, np.float32), np.zeros(3, np.float32), [5])[1]).all()
    assert np.isinf(degrade_ref.noise(x, np.zeros(3, np.float32), [5])[1]).all()


# ---- the exports -----------------------------------------------------------------------------------------------------------------
def test_the_three_entry_points_are_bound_and_exported(built_lib):
    from nomad_amd import _lib
    counts = {"nomad_degrade_scratch_bytes": 3, "nomad_degrade_noise": 14, "nomad_degrade_clip": 12}
    lib = C.CDLL(built_lib)
    for name, n in counts.items():
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.SIGNATURES["nomad_degrade_scratch_bytes"][0] is C.c_size_t
    loaded = _lib.load()
    assert loaded.nomad_degrade_scratch_bytes(2, 1028, 7) >= 2 * 2 * 1028 * 4 + 2 * 7 * 2 * 8
    assert loaded.nomad_degrade_scratch_bytes(2, 1026, 7) == 0 and loaded.nomad_last_error()
    # without a context the calls are refused before anything else happens
    assert loaded.nomad_degrade_clip(None, None, 1, 4, None, None, 1, None, None, None, 0, None) == _lib.NOMAD_ERR_INVALID
    assert loaded.nomad_degrade_noise(None, None, 1, 4, None, None, 1, None, 1, None, None, None, 0, None) == _lib.NOMAD_ERR_INVALID


# ---- a recording fake engine -----------------------------------------------------------------------------------------------------
class _SweepEngine:
    """Clip i holds the value i + 1; a degraded row holds its clip's value + level / 1000; a row is "embedded" as [that value, 0, ...]
    and the references are zeros - so a row's score is its value and tells which clip at which level it is."""
    device = torch.device("cpu")
    encoder_depth = 12

    def __init__(self):
        self.calls = []

    def pack_ragged_host(self, waves):
        flat = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lens = [int(w.numel()) for w in flat]
        host = torch.zeros(len(flat), (max(lens) + 3) // 4 * 4)
        for i, w in enumerate(flat):
            host[i, :lens[i]] = w
        return host, lens

    def _pack(self, waves, packed=None):
        self.calls.append(("upload", list(packed[1])))
        return packed

    def pack_ragged(self, waves, lengths=None):
        if lengths is not None:
            return waves, [int(n) for n in lengths]
        return self.pack_ragged_host(waves)

    def _degrade(self, kind, buf, levels, lengths):
        self.calls.append((kind, list(lengths), [float(v) for v in levels]))
        G = len(levels)
        out = torch.zeros(buf.shape[0] * G, buf.shape[1])
        for b in range(buf.shape[0]):
            for g, v in enumerate(levels):
                out[b * G + g, :lengths[b]] = buf[b, 0] + float(v) / 1000
        return out, [n for n in lengths for _ in range(G)], None

    def degrade_noise(self, buf, noise, levels, lengths=None):
        assert torch.is_tensor(noise) and noise.dim() == 1
        return self._degrade("noise", buf, levels, lengths)

    def degrade_clip(self, buf, levels, lengths=None):
        return self._degrade("clip", buf, levels, lengths)

    def embed_ragged(self, waves, precision=None, packed=None):
        out, lens = packed
        assert waves is None and out.shape[0] == len(lens)
        self.calls.append(("embed", sum(lens), precision))
        emb = torch.zeros(len(lens), 256)
        emb[:, 0] = out[:, 0]
        return emb

    def fetch_async(self, t):
        class F:
            def result(self_inner):
                return t.numpy()
        return F()

    @staticmethod
    def _dist(a, b):
        return (a[:, :1].double() - b[:, 0].double()[None, :]).abs()

    def pairwise(self, deg, ref, want_matrix=True):
        self.calls.append(("pairwise", deg.shape[0]))
        d = self._dist(deg, ref)
        return d, d.mean(1)

    def knn(self, a, b, k, want_matrix=False):
        self.calls.append(("knn", a.shape[0], k))
        return knn_ref(self._dist(a, b), k)


def _nomad(engine):
    n = Nomad.__new__(Nomad)            # no GPU: only the host side is under test
    n.engine, n.precision, n.group = engine, "fp32", None
    return n


REFS = torch.zeros(3, 256)
LENS = [1000, 1000, 1000, 3000]


def _clean():
    x = torch.zeros(4, 3000)
    for b, n in enumerate(LENS):
        x[b, :n] = b + 1
    return x


def test_degrade_rows_lengths_and_refusals():
    eng = _SweepEngine()
    n = _nomad(eng)
    noise = torch.ones(7)
    rows, lens = n.degrade(_clean().unsqueeze(1), "noise", [0, 15, 40], noise=noise, lengths=LENS)
    assert rows.shape == (12, 3000) and lens == [1000] * 9 + [3000] * 3
    assert eng.calls == [("noise", LENS, [0.0, 15.0, 40.0])]
    assert torch.allclose(rows[:, 0], torch.tensor([b + 1 + v / 1000 for b in range(4) for v in (0, 15, 40)], dtype=torch.float32))
    rows, lens = n.degrade(_clean(), "clip", [5])
    assert rows.shape == (4, 3000) and lens == [3000] * 4 and eng.calls[-1] == ("clip", [3000] * 4, [5.0])
    eng.calls.clear()
    with pytest.raises(ValueError, match="noise signal"):
        n.degrade(_clean(), "noise", [5])
    with pytest.raises(ValueError, match="goes with kind 'noise'"):
        n.degrade(_clean(), "clip", [5], noise=noise)
    with pytest.raises(ValueError, match="'noise' or 'clip'"):
        n.degrade(_clean(), "reverb", [5])
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.degrade(torch.zeros(3000), "clip", [5])
    with pytest.raises(ValueError, match="produces no gradient"):
        n.degrade(_clean().requires_grad_(True), "clip", [5])
    with pytest.raises(ValueError, match="produces no gradient"):
        n.degrade(_clean(), "noise", [5], noise=noise.clone().requires_grad_(True))
    assert eng.calls == []


@pytest.mark.parametrize("k", [None, 2])
def test_intensity_sweep_row_order_batches_and_statistics(k, capsys):
    eng = _SweepEngine()
    n = _nomad(eng)
    snr, cf = [40, 0, 15], [5, 60]
    res = n.intensity_sweep(_clean(), REFS, noise=torch.ones(5), snr_db=snr, clip_factor=cf, lengths=LENS, k=k, max_batch_samples=6000)
    # 6000 samples over G = 3 rows per clip: batches of at most 2000 clean samples, one clip at least
    cuts = [[1000, 1000], [1000], [3000]]
    want = []
    for lens in cuts:
        want += [("noise", lens, [40.0, 0.0, 15.0]), ("embed", 3 * sum(lens), "fp32"), ("clip", lens, [5.0, 60.0]), ("embed", 2 * sum(lens), "fp32")]
    dist = ("knn", 12, 2) if k else ("pairwise", 12)
    assert eng.calls == want + [dist, ("knn", 8, 2) if k else ("pairwise", 8)]
    assert sorted(res) == ["CLIP", "NOISE"]
    for name, levels in (("NOISE", snr), ("CLIP", cf)):
        r = res[name]
        assert sorted(r) == ["SRCC", "embeddings", "scores", "table"]
        assert np.allclose(r["scores"], [b + 1 + v / 1000 for b in range(4) for v in levels], atol=1e-6), "row b G + g is clip b at level g"
        assert list(r["table"].columns) == ["Condition", "Distance"]
        t = r["table"].sort_values(by="Condition")
        assert t["Condition"].tolist() == sorted(float(v) for v in levels)
        assert np.allclose(t["Distance"], [2.5 + v / 1000 for v in sorted(levels)], atol=1e-6)
        assert r["SRCC"] == pytest.approx(1.0)
        again = T.intensity_stats(r["embeddings"], pd.DataFrame({"filepath_deg": r["embeddings"]["filepath_deg"],
                                                                 "Condition": [float(v) for v in levels] * 4}),
                                  pd.DataFrame(REFS.numpy()), lambda a, b: r["scores"], name)
        assert again["table"].equals(r["table"]) and again["SRCC"] == r["SRCC"]
    # one degradation alone; the other is left out
    eng.calls.clear()
    only = n.intensity_sweep(_clean(), REFS, clip_factor=cf, lengths=LENS)
    assert sorted(only) == ["CLIP"] and eng.calls == [("clip", LENS, [5.0, 60.0]), ("embed", 12000, "fp32"), ("pairwise", 8)]
    # a list of clips is a batch as well
    eng.calls.clear()
    n.intensity_sweep([torch.full((700,), 1.0), np.full(500, 2.0, dtype=np.float32)], REFS, clip_factor=[5])
    assert eng.calls[0] == ("clip", [700, 500], [5.0])


def test_intensity_sweep_refusals():
    eng = _SweepEngine()
    n = _nomad(eng)
    with pytest.raises(ValueError, match="needs a noise signal"):
        n.intensity_sweep(_clean(), REFS, snr_db=[0, 15])
    with pytest.raises(ValueError, match="snr_db, clip_factor or both"):
        n.intensity_sweep(_clean(), REFS, noise=torch.ones(4))
    with pytest.raises(ValueError, match="1 .. 64 levels"):
        n.intensity_sweep(_clean(), REFS, clip_factor=list(range(65)))
    with pytest.raises(ValueError, match="produces no gradient"):
        n.intensity_sweep(_clean().requires_grad_(True), REFS, clip_factor=[5])
    with pytest.raises(ValueError, match="produces no gradient"):
        n.intensity_sweep(_clean(), REFS.clone().requires_grad_(True), clip_factor=[5])
    with pytest.raises(ValueError, match="k = 4"):
        n.intensity_sweep(_clean(), REFS, clip_factor=[5], k=4)
    with pytest.raises(ValueError, match="lengths"):
        n.intensity_sweep(_clean(), REFS, clip_factor=[5], lengths=[100, 1000, 1000, 3000])     # shorter than one encoder frame
    eng.encoder_depth = 6
    with pytest.raises(RuntimeError, match="whole encoder"):
        n.intensity_sweep(_clean(), REFS, clip_factor=[5])
    assert eng.calls == []


def test_intensity_sweep_over_files_uploads_each_batch_once(tmp_path, capsys):
    sizes = {"a": 1000, "b": 1200, "c": 900}
    for name in sizes:
        (tmp_path / f"{name}.wav").write_bytes(b"")
    eng = _SweepEngine()
    n = _nomad(eng)
    n.load_processing = lambda p, trim=False: np.full((1, sizes[os.path.basename(p)[:-4]]), float(sizes[os.path.basename(p)[:-4]]), np.float32)
    n.NATIVE_WAV_THREADS = 0            # the files are empty: everything goes through load_processing
    res = n.intensity_sweep(str(tmp_path), REFS, noise=torch.ones(5), snr_db=[0, 20], clip_factor=[5, 10, 50], max_batch_samples=10 ** 6)
    order = [sizes[f[:-4]] for f in os.listdir(tmp_path)]
    assert eng.calls[:5] == [("upload", order), ("noise", order, [0.0, 20.0]), ("embed", 2 * sum(order), "fp32"),
                             ("clip", order, [5.0, 10.0, 50.0]), ("embed", 3 * sum(order), "fp32")]
    assert np.allclose(res["CLIP"]["scores"], [s + v / 1000 for s in order for v in (5, 10, 50)], rtol=1e-6)
    names = list(res["NOISE"]["embeddings"]["filepath_deg"])
    assert len(set(names)) == 6 and all(str(tmp_path) in x for x in names)
    with pytest.raises(ValueError, match="lengths go with tensors"):
        n.intensity_sweep(str(tmp_path), REFS, clip_factor=[5], lengths=[1, 2, 3])
    csv = tmp_path / "list.csv"
    pd.DataFrame({"filename": [str(tmp_path / "b.wav")]}).to_csv(csv, index=False)
    eng.calls.clear()
    n.intensity_sweep(str(csv), REFS, clip_factor=[5])
    assert eng.calls[:2] == [("upload", [1200]), ("clip", [1200], [5.0])]


# ---- Training.eval_degradation_intensity -----------------------------------------------------------------------------------------
def _training(config, calls, nomad=None):
    rng = np.random.default_rng(2)
    t = T.Training.__new__(T.Training)
    t.config, t.model, t.nomad = config, "model", nomad
    t._load_model = lambda path, allow_w2v: calls.append(("load", path, allow_w2v))
    ref = pd.concat([pd.DataFrame({"reference": [f"nmr/r{i}.wav" for i in range(4)]}),
                     pd.DataFrame(rng.standard_normal((4, 256)).astype(np.float32))], axis=1)
    t.get_nmr_embeddings = lambda: calls.append(("nmr",)) or ref.copy()

    def emb(model, names, root=False):
        calls.append(("embed", model, list(names), root))
        names = pd.DataFrame({"filepath_deg": list(names)})
        return pd.concat([names, pd.DataFrame(rng.standard_normal((len(names), 256)).astype(np.float32))], axis=1)

    t.get_embeddings_csv = emb
    t._nmr_mean = lambda a, b: np.linalg.norm(a[:, None, :].astype(np.float64) - b[None].astype(np.float64), axis=2).mean(1)
    return t


def test_eval_degradation_intensity_without_the_key_is_the_file_path(tmp_path, capsys):
    rows = [dict(Degradation=d, Condition=c, filepath_deg=f"{d}_{c}.wav") for d in ("clip", "noise") for c in (1, 2, 3)]
    pd.DataFrame(rows).to_csv(tmp_path / "mono.csv", index=False)
    calls = []

    class _NoSweep:
        def intensity_sweep(self, *a, **kw):
            pytest.fail("the file path called intensity_sweep")

    t = _training({"test_mono_data": str(tmp_path / "mono.csv"), "test_mono_wav": "/wav"}, calls, _NoSweep())
    res = t.eval_degradation_intensity("model.pt")
    assert calls == [("load", "model.pt", True), ("nmr",),
                     ("embed", "model", [f"clip_{c}.wav" for c in (1, 2, 3)], "/wav"),
                     ("embed", "model", [f"noise_{c}.wav" for c in (1, 2, 3)], "/wav")]
    assert sorted(res) == ["clip", "noise"] and sorted(res["clip"]) == ["SRCC", "embeddings", "ref_embeddings", "table"]


def test_eval_degradation_intensity_on_the_device(capsys):
    calls, seen = [], {}

    class _Sweep:
        def load_processing(self, path, *a, **kw):
            seen["noise_path"] = path
            return torch.arange(6, dtype=torch.float32).reshape(1, 6)

        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, **kw):
            seen.update(clean=clean, refs=references, noise=noise, snr_db=snr_db, clip=clip_factor, kw=kw)
            table = pd.DataFrame({"Condition": [1.0, 2.0], "Distance": [0.5, 0.6]})
            return {name: dict(table=table, SRCC=1.0, embeddings=pd.DataFrame(), scores=np.zeros(2)) for name in ("NOISE", "CLIP")}

    cfg = {"degrade_on_device": {"clean": "/clean", "noise": "/noise.wav", "snr_db": [0, 15], "clip": [5, 40]}}
    t = _training(cfg, calls, _Sweep())
    res = t.eval_degradation_intensity("model.pt")
    assert calls == [("load", "model.pt", True), ("nmr",)]                     # no test_mono_data, no rendered file
    assert seen["clean"] == "/clean" and seen["noise_path"] == "/noise.wav" and seen["noise"].tolist() == [0, 1, 2, 3, 4, 5]
    assert seen["snr_db"] == [0, 15] and seen["clip"] == [5, 40] and seen["kw"] == {}
    assert tuple(seen["refs"].shape) == (4, 256) and seen["refs"].dtype == torch.float32
    assert sorted(res) == ["CLIP", "NOISE"]
    for r in res.values():                                                      # the shape of the file path's result, and the rows' scores
        assert {"SRCC", "embeddings", "ref_embeddings", "table"} <= set(r)
        assert list(r["ref_embeddings"].index) == [f"nmr/r{i}.wav" for i in range(4)]
    t = _training({"degrade_on_device": {"clean": "/clean", "clip": [5]}}, calls, _Sweep())
    seen.clear()
    t.eval_degradation_intensity("model.pt")
    assert seen["noise"] is None and seen["snr_db"] is None and "noise_path" not in seen
    t = _training(dict(cfg, eval_w2v=True), [], _Sweep())
    with pytest.raises(ValueError, match="eval_w2v"):
        t.eval_degradation_intensity("model.pt")


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,word", [(["--sweep", "--clip", "5", "--window", "2"], "--window"),
                                        (["--sweep"], "levels"),
                                        (["--sweep", "--snr-db", "0,15"], "--noise"),
                                        (["--sweep", "--noise", "n.wav", "--clip", "5"], "--noise"),
                                        (["--sweep", "--clip", "5,abc"], "--clip"),
                                        (["--sweep", "--clip", "5,nan"], "--clip"),
                                        (["--sweep", "--clip", "101"], "--clip"),
                                        (["--sweep", "--clip", ",".join(["5"] * 65)], "--clip"),
                                        (["--clip", "5"], "--sweep"),
                                        (["--noise", "n.wav"], "--sweep")])
def test_cli_argument_errors(extra, word, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_sweep_writes_the_intensity_table(tmp_path, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    nmr, deg, out = tmp_path / "nmr", tmp_path / "clean", tmp_path / "out"
    for d in (nmr, deg, out):
        d.mkdir()
    seen = {}

    class _Fake:
        def __init__(self, **kw):
            pass

        def get_embeddings(self, path):
            return pd.concat([pd.DataFrame({"filename": ["r0", "r1"]}), pd.DataFrame(np.ones((2, 256), dtype=np.float32))], axis=1)

        def load_processing(self, path, *a, **kw):
            return torch.ones(1, 9)

        def predict(self, *a, **kw):
            pytest.fail("--sweep called predict")

        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, k=None):
            seen.update(clean=clean, refs=tuple(references.shape), noise=noise, snr_db=snr_db, clip=clip_factor, k=k)
            return {"NOISE": dict(table=pd.DataFrame({"Condition": [15.0, 0.0], "Distance": [0.25, 0.75]}), SRCC=-1.0),
                    "CLIP": dict(table=pd.DataFrame({"Condition": [5.0, 40.0], "Distance": [0.3, 0.4]}), SRCC=1.0)}

    monkeypatch.setattr(cli, "Nomad", _Fake)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--mode", "dir", "--nmr", str(nmr), "--deg", str(deg), "--results_path", str(out),
                                      "--sweep", "--noise", "n.wav", "--snr-db", "0,15", "--clip", "5,40", "--knn", "2"])
    cli.main()
    assert seen == dict(clean=str(deg), refs=(2, 256), noise=seen["noise"], snr_db=[0.0, 15.0], clip=[5.0, 40.0], k=2)
    assert seen["noise"].shape == (9,)
    assert os.listdir(out) == ["nomad_intensity.csv"]
    back = pd.read_csv(out / "nomad_intensity.csv")
    assert list(back.columns) == ["Degradation", "Condition", "NOMAD"]
    assert back.to_dict("list") == {"Degradation": ["NOISE", "NOISE", "CLIP", "CLIP"], "Condition": [0.0, 15.0, 5.0, 40.0],
                                    "NOMAD": [0.75, 0.25, 0.3, 0.4]}
    printed = capsys.readouterr().out
    assert "NOISE: SRCC" in printed and "-1.000" in printed and "CLIP: SRCC" in printed
