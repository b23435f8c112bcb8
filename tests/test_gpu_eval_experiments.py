"""GPU: the reference's four evaluation experiments (src/training/train_triplet.py:231-474) on the engine, with the NOMAD model and
with the raw wav2vec 2.0 baseline (``eval_w2v: True``, ``Origw2v``).

The reference's own ``Training`` class cannot run here (it imports fairseq at module level), so the tests restate its pandas /
SciPy lines on the engine's own embeddings.  A synthetic database is written into ``tmp_path``: 16 kHz PCM-16 wavs of 1-3 s; 5
clean non-matching references; 2 databases x 6 conditions x 4 files, a condition being a noise level from {0, 0.003, 0.01, 0.03,
0.1, 0.3} added to a clean base of modulated noise, ``mos`` falling with the level plus a seeded jitter; a matching clean
reference per degraded file; CSVs with the reference's column names.  Weights: ``seeded``.

Per experiment:
* the returned per-file embeddings equal one ``engine.embed`` / ``embed_features`` call per clip (``torch.equal``: the ragged
  guarantee);
* the per-condition ``Distance`` column is within ``1e-13 * max(1, value)`` of ``scipy.spatial.distance.cdist`` + pandas on those
  embeddings (``np.diag`` of the matrix for quality_fr): the float64 bound of tests/test_gpu_cdist.py at D <= 768;
* ``Distance_map``, ``popt``, SRCC and PCC are compared with ``curve_fit`` / ``spearmanr`` / ``pearsonr`` applied by the test to the
  returned ``Distance`` and ``mos`` columns - the same functions on the same numbers in the same process, so 1e-12;
* before SRCC is compared, the smallest gap between two conditions' mean distances in the test's own SciPy recomputation must
  exceed 1e-9 and every database must have at least 4 conditions (a cubic needs them): a rank correlation cannot then pass by
  accident or fail by a tie.  An inconclusive database fails the test."""
import os
import struct

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.optimize import curve_fit
from scipy.spatial.distance import cdist
from scipy.stats import pearsonr, spearmanr

pytestmark = pytest.mark.gpu

LEVELS = [0.0, 0.003, 0.01, 0.03, 0.1, 0.3]
DBS = ["dbA", "dbB"]
MIN_GAP = 1e-9


def _write_wav(path, x, sr=16000):
    pcm = (np.clip(x, -1, 1) * 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(pcm)) + pcm)


def _clean(rng, n):
    """Noise under a slow envelope: something with structure in time, 0.1 rms at most."""
    t = np.arange(n) / 16000.0
    env = 0.55 + 0.45 * np.sin(2 * np.pi * (1.5 + 3 * rng.rand()) * t + 2 * np.pi * rng.rand())
    return 0.1 * env * rng.randn(n)


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    root = tmp_path_factory.mktemp("evaldb")
    rng = np.random.RandomState(11)
    for d in ["nmr", "test", "mono", "val", "out"] + [f"test/{db}" for db in DBS]:
        os.makedirs(root / d, exist_ok=True)
    for i in range(5):
        _write_wav(str(root / "nmr" / f"clean_{i}.wav"), _clean(rng, 16000 + 4000 * i))
    rows = []
    for db in DBS:
        for k, level in enumerate(LEVELS):
            for f in range(4):
                n = int(16000 * (1 + 2 * rng.rand()))
                base = _clean(rng, n)
                deg, ref = f"{db}/deg_c{k}_{f}.wav", f"{db}/ref_c{k}_{f}.wav"
                _write_wav(str(root / "test" / ref), base)
                _write_wav(str(root / "test" / deg), base + level * rng.randn(n))
                rows.append(dict(db=db, condition=f"{db}_c{k}", mos=4.7 - 0.65 * k + 0.05 * rng.randn(), filepath_deg=deg,
                                 filepath_ref=ref))
    test_csv = str(root / "test.csv")
    pd.DataFrame(rows).sample(frac=1.0, random_state=1).to_csv(test_csv, index=False)
    mono = []
    for degr, amp in (("noise", 0.02), ("hum", 0.05)):
        for cond in range(1, 6):
            for f in range(3):
                n = 16000 + 3000 * f
                t = np.arange(n) / 16000.0
                add = rng.randn(n) if degr == "noise" else np.sign(np.sin(2 * np.pi * 100 * t))
                name = f"{degr}_{cond}_{f}.wav"
                _write_wav(str(root / "mono" / name), _clean(rng, n) + amp * cond * add)
                mono.append(dict(Degradation=degr, Condition=cond, filepath_deg=name))
    mono_csv = str(root / "mono.csv")
    pd.DataFrame(mono).to_csv(mono_csv, index=False)
    val = []
    for spk in range(3):
        for kind, amp in (("clean", 0.0), ("noise", 0.05), ("loud", 0.25)):
            name = f"val/spk{spk}_{kind}_{int(amp * 100)}.wav"
            n = 17000 + 2500 * spk
            _write_wav(str(root / name), _clean(rng, n) + amp * rng.randn(n))
            val.append(dict(Anchor=name, Positive=name, Negative=name, db=1 + spk % 2))
    val_csv = str(root / "val.csv")
    pd.DataFrame(val).to_csv(val_csv, index=False)
    return dict(root=root, test_csv=test_csv, mono_csv=mono_csv, val_csv=val_csv)


def _config(database, name, **over):
    root = database["root"]
    cfg = dict(experiment_name=name, out_dir=str(root / "out"), training_script="src.training.train_triplet",
               checkpoint_path="seeded", nomad_model_path="seeded", ssl_out_dim=768, emb_dim=256, eval_w2v=False,
               non_match_dir=str(root / "nmr"), test_db_file=database["test_csv"], test_db_file_fr=database["test_csv"],
               test_root_wav=str(root / "test"), db=None, conds=None, test_mono_data=database["mono_csv"],
               test_mono_wav=str(root / "mono"), root=str(root), valid_df=database["val_csv"], current_level=[1, 2], trim=False)
    cfg.update(over)
    return cfg


def _training(database, engine, name, **over):
    from nomad_amd.train import Training
    return Training(_config(database, name, **over), engine=engine)


def _per_clip(engine, tr, paths, w2v):
    """One uniform call per file - what the ragged pipeline must reproduce bit for bit."""
    out = []
    for p in paths:
        wav = tr.nomad.load_processing(p).to(engine.device, torch.float32).contiguous()
        out.append(engine.embed_features(wav) if w2v else engine.embed(wav))
    return torch.cat(out).cpu()


def _same_embeddings(engine, tr, df_emb, column, root, w2v):
    width = 768 if w2v else 256
    assert df_emb.shape[1] == 1 + width and list(df_emb.columns[1:]) == list(range(width))
    got = torch.from_numpy(np.ascontiguousarray(df_emb.iloc[:, 1:].to_numpy(dtype=np.float32)))
    paths = [os.path.join(root, n) if root else n for n in df_emb[column]]
    want = _per_clip(engine, tr, paths, w2v)
    assert torch.equal(got, want), f"{int((got != want).any(1).sum())} of {len(paths)} files differ from their own call"


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = 1e-13 * np.maximum(1.0, np.abs(want))
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all(), f"{what}: worst {np.abs(got - want).max():.3e}"


def _order_three(x, a, b, c, d):
    return a * x + b * x ** 2 + c * x ** 3 + d


def _check_mos(res, want_dist, what):
    """want_dist: the test's own per-condition table (SciPy distances, pandas grouping)."""
    table = res["table"]
    assert list(table.index) == list(want_dist.index), what
    assert len(table) >= 4, f"{what}: a cubic needs at least 4 conditions"
    gap = np.diff(np.sort(want_dist["Distance"].values)).min()
    print(f"EVAL {what}: {len(table)} conditions, smallest gap between mean distances {gap:.3e}")
    assert gap > MIN_GAP, f"{what}: conditions {gap:.3e} apart - inconclusive for a rank correlation"
    _close(table["Distance"].values, want_dist["Distance"].values, what + " Distance")
    _close(table["mos"].values, want_dist["mos"].values, what + " mos")
    popt, _ = curve_fit(_order_three, table["Distance"].values, table["mos"].values)
    dmap = table["Distance"].apply(lambda x: _order_three(x, *popt))
    np.testing.assert_allclose(res["popt"], popt, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(table["Distance_map"].values, dmap.values, rtol=1e-12, atol=1e-12)
    assert abs(res["SRCC"] - spearmanr(table["Distance"], table["mos"])[0]) <= 1e-12
    assert abs(res["SRCC_map"] - spearmanr(dmap, table["mos"])[0]) <= 1e-12
    assert abs(res["PCC"] - pearsonr(table["Distance"], table["mos"])[0]) <= 1e-12
    assert abs(res["PCC_map"] - pearsonr(dmap, table["mos"])[0]) <= 1e-12


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except Exception:  # noqa: BLE001
        return False


@pytest.mark.parametrize("w2v", [False, True], ids=["nomad", "w2v"])
def test_quality_nmr(database, engine, w2v, capsys):
    tr = _training(database, engine, "quality_nmr", eval_w2v=w2v)
    results = tr.eval_audio_quality("seeded")
    out = capsys.readouterr().out
    assert sorted(results) == DBS and not engine.train_enabled
    data = pd.read_csv(database["test_csv"])
    for db_name, db in data.groupby("db"):
        res = results[db_name]
        _same_embeddings(engine, tr, res["embeddings"], "filepath_deg", str(database["root"] / "test"), w2v)
        _same_embeddings(engine, tr, res["ref_embeddings"].reset_index(), "reference", None, w2v)
        # train_triplet.py:262-274 on the returned embeddings
        df_emb, ref = res["embeddings"], res["ref_embeddings"]
        assert len(ref) == 5 and len(df_emb) == 24
        test_embeddings = df_emb.set_index("filepath_deg")
        test_names = df_emb.merge(db, on="filepath_deg")[["filepath_deg", "condition", "mos"]]
        avg = np.mean(cdist(test_embeddings, ref), axis=1)
        df_dist = pd.DataFrame({"filepath_deg": test_embeddings.index, "Distance": avg})
        df_dist = df_dist.merge(test_names, on="filepath_deg").set_index("filepath_deg").groupby("condition").mean()
        _check_mos(res, df_dist, f"quality_nmr[{'w2v' if w2v else 'nomad'}] {db_name}")
        if _have_matplotlib():
            assert res["figure"] == os.path.join(str(database["root"] / "out"), f"{db_name}_embeddings.png")
            assert os.path.getsize(res["figure"]) > 1000
    for line in ("SRCC: ", "SRCC 3rd map: ", "PCC: ", "PCC 3rd map: "):
        assert out.count(line) == 2, line
    assert "dbA" in out and "dbB" in out


def test_quality_nmr_filters(database, engine):
    tr = _training(database, engine, "quality_nmr", db=["dbB"], conds=["c0", "c2", "c3", "c5"])
    results = tr.eval_audio_quality("seeded")
    assert list(results) == ["dbB"]
    assert list(results["dbB"]["table"].index) == ["dbB_c0", "dbB_c2", "dbB_c3", "dbB_c5"] and len(results["dbB"]["embeddings"]) == 16


def test_quality_fr(database, engine, capsys):
    tr = _training(database, engine, "quality_fr")
    results = tr.eval_full_reference("seeded")
    out = capsys.readouterr().out
    assert sorted(results) == DBS and not engine.train_enabled
    data = pd.read_csv(database["test_csv"])
    for db_name, db in data.groupby("db"):
        res = results[db_name]
        root = str(database["root"] / "test")
        _same_embeddings(engine, tr, res["embeddings"], "filepath_deg", root, False)
        _same_embeddings(engine, tr, res["ref_embeddings"], "filepath_ref", root, False)
        # train_triplet.py:433-445 on the returned embeddings
        e_ref, e_test = res["ref_embeddings"].set_index("filepath_ref"), res["embeddings"].set_index("filepath_deg")
        test_names = res["embeddings"].merge(db, on="filepath_deg")[["filepath_deg", "condition", "mos"]]
        fr = np.diag(cdist(e_test, e_ref))
        df_dist = pd.DataFrame({"filepath_deg": e_test.index, "Distance": fr}).merge(test_names, on="filepath_deg")
        df_dist = df_dist.groupby("condition")[["Distance", "mos"]].mean()
        assert df_dist["Distance"].iloc[0] == 0.0          # noise level 0: the degraded file is its reference
        _check_mos(res, df_dist, f"quality_fr {db_name}")
        if _have_matplotlib():
            assert res["figure"] == os.path.join(str(database["root"] / "out"), f"fr_{db_name}_embeddings.png")
            assert os.path.getsize(res["figure"]) > 1000
    assert out.count("SRCC: ") == 2 and out.count("PCC 3rd map: ") == 2


@pytest.mark.parametrize("w2v", [False, True], ids=["nomad", "w2v"])
def test_intensity(database, engine, w2v, capsys):
    tr = _training(database, engine, "intensity", eval_w2v=w2v)
    results = tr.eval_degradation_intensity("seeded")
    out = capsys.readouterr().out
    assert sorted(results) == ["hum", "noise"] and not engine.train_enabled
    data = pd.read_csv(database["mono_csv"])
    for deg_name, deg_data in data.groupby("Degradation"):
        res = results[deg_name]
        _same_embeddings(engine, tr, res["embeddings"], "filepath_deg", str(database["root"] / "mono"), w2v)
        # train_triplet.py:371-390 on the returned embeddings
        df_emb, ref = res["embeddings"], res["ref_embeddings"]
        test_embeddings = df_emb.set_index("filepath_deg")
        test_names = df_emb.merge(deg_data, on="filepath_deg")[["filepath_deg", "Condition"]]
        avg = np.mean(cdist(test_embeddings, ref), axis=1)
        df_dist = pd.DataFrame({"filepath_deg": test_embeddings.index, "Distance": avg}).merge(test_names, on="filepath_deg")
        df_dist.set_index("filepath_deg", inplace=True)
        df_dist = df_dist.groupby("Condition").mean().reset_index()
        df_dist.sort_values(by="Distance", inplace=True)
        what = f"intensity[{'w2v' if w2v else 'nomad'}] {deg_name}"
        gap = np.diff(df_dist["Distance"].values).min()
        print(f"EVAL {what}: smallest gap between mean distances {gap:.3e}")
        assert len(df_dist) >= 4 and gap > MIN_GAP, f"{what}: inconclusive"
        assert list(res["table"]["Condition"]) == list(df_dist["Condition"])
        _close(res["table"]["Distance"].values, df_dist["Distance"].values, what)
        assert abs(res["SRCC"] - spearmanr(res["table"]["Distance"], res["table"]["Condition"])[0]) <= 1e-12
    assert "Degradation: hum" in out and "Degradation: noise" in out and out.count("SRCC: ") == 2


def test_valid_rank(database, engine):
    tr = _training(database, engine, "valid_rank")
    res = tr.eval_degr_level("seeded")
    assert not engine.train_enabled
    _same_embeddings(engine, tr, res["embeddings"], "Anchor", str(database["root"]), False)
    _same_embeddings(engine, tr, res["ref_embeddings"], "reference", None, False)
    # train_triplet.py:317-333 on the returned embeddings
    df_emb, ref = res["embeddings"], res["ref_embeddings"]
    assert len(df_emb) == 9
    avg = np.mean(cdist(df_emb.iloc[:, 1:].to_numpy(), ref.iloc[:, 1:].to_numpy()), axis=1)
    df_dist = pd.DataFrame({"Anchor": df_emb["Anchor"], "Distance": avg})
    df_dist.sort_values(by="Distance", inplace=True)
    df_dist["condition"] = [x.split("_")[1] + " " + x.split("_")[2].split(".")[0] for x in df_dist["Anchor"]]
    order = df_dist.groupby("condition")["Distance"].mean().sort_values()
    assert np.diff(np.sort(avg)).min() > MIN_GAP and np.diff(order.values).min() > MIN_GAP, "valid_rank: inconclusive"
    assert list(res["table"]["Anchor"]) == list(df_dist["Anchor"]) and list(res["table"]["condition"]) == list(df_dist["condition"])
    _close(res["table"]["Distance"].values, df_dist["Distance"].values, "valid_rank Distance")
    assert res["order"] == list(order.index) and sorted(res["order"]) == ["clean 0", "loud 25", "noise 5"]
    if _have_matplotlib():
        assert res["figure"] == os.path.join(str(database["root"] / "out"), "validset_embeddings.png")
        assert os.path.getsize(res["figure"]) > 1000


@pytest.mark.parametrize("name,method", [("valid_rank", "eval_degr_level"), ("quality_fr", "eval_full_reference")])
def test_w2v_is_refused_where_the_reference_loads_unconditionally(database, engine, name, method):
    tr = _training(database, engine, name, eval_w2v=True)
    with pytest.raises(ValueError, match="eval_w2v"):
        getattr(tr, method)("seeded")
    assert not engine.train_enabled


def test_model_path_is_a_nomad_layout_checkpoint(database, engine, sd0, built_lib):
    """nomad_model_path as a file (what Training.save writes): the engine is built from it, with no optimiser state, and the
    figure goes next to it."""
    from nomad_amd.train import Training
    ckpt_dir = database["root"] / "ckpt"
    os.makedirs(ckpt_dir, exist_ok=True)
    path = str(ckpt_dir / "best_model.pt")
    torch.save(sd0, path)
    tr = Training(_config(database, "quality_nmr", nomad_model_path=path, checkpoint_path="unused", db=["dbA"]))
    try:
        assert tr.engine is None
        results = tr.eval_audio_quality(path)
        assert not tr.engine.train_enabled
        _same_embeddings(engine, tr, results["dbA"]["embeddings"], "filepath_deg", str(database["root"] / "test"), False)
        if _have_matplotlib():
            assert results["dbA"]["figure"] == os.path.join(str(ckpt_dir), "dbA_embeddings.png") and os.path.isfile(results["dbA"]["figure"])
    finally:
        torch.cuda.synchronize()
        if tr.engine is not None:
            tr.engine.close()


def test_main_runs_quality_nmr_from_a_yaml_file(database, engine, tmp_path, capsys):
    import yaml
    from nomad_amd import train
    cfg = str(tmp_path / "eval.yaml")
    with open(cfg, "w") as f:
        yaml.dump(_config(database, "quality_nmr", precision="fp32"), f)
    results = train.main(["--config_file", cfg])
    out = capsys.readouterr().out
    assert sorted(results) == DBS and out.count("SRCC: ") == 2
    ref = _training(database, engine, "quality_nmr").eval_audio_quality("seeded")
    for db in DBS:
        assert results[db]["table"].equals(ref[db]["table"])          # a second engine on the same weights: the same bits
    with pytest.raises(SystemExit):
        with open(cfg, "w") as f:
            yaml.dump(_config(database, "quality_xyz"), f)
        train.main(["--config_file", cfg])
