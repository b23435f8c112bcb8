"""CPU: the host side of the evaluation experiments (nomad_amd/train.py: quality_nmr, valid_rank, intensity, quality_fr).

The statistics stage is a set of pure functions - embedding tables in, result dict out, distances from an injected function -
and is compared here with a direct restatement of the reference's pandas / SciPy lines (src/training/train_triplet.py:231-474)
on random embeddings, the distances coming from ``scipy.spatial.distance.cdist`` on both sides.  ``main`` dispatches every
experiment name of the reference's main.py, and ``Nomad.get_embeddings_csv`` yields 768 columns for an ``Origw2v`` model."""
import os

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.optimize import curve_fit
from scipy.spatial.distance import cdist
from scipy.stats import pearsonr, spearmanr

from nomad_amd import train as T


def _nmr_mean(test, ref):
    return np.mean(cdist(test, ref), axis=1)


def _paired(test, ref):
    return np.diag(cdist(test, ref))


def _emb_table(names, column, dim, rng, shift=None):
    """What get_embeddings_csv returns: the name column, then integer-named fp32 embedding columns."""
    e = rng.standard_normal((len(names), dim)).astype(np.float32)
    if shift is not None:
        e += np.asarray(shift, dtype=np.float32)[:, None]
    return pd.concat([pd.DataFrame({column: list(names)}), pd.DataFrame(e)], axis=1)


def _database(rng, dbs=("dbA", "dbB", "dbC"), conds=6, files=4):
    rows = []
    for db in dbs:
        for c in range(conds):
            for f in range(files):
                rows.append(dict(db=db, condition=f"{db}_c{c}", mos=4.6 - 0.6 * c + 0.1 * rng.standard_normal(),
                                 filepath_deg=f"{db}/deg_c{c}_{f}.wav", filepath_ref=f"{db}/ref_c{c}_{f}.wav"))
    return pd.DataFrame(rows).sample(frac=1.0, random_state=3).reset_index(drop=True)     # not in condition order


def _order_three(x, a, b, c, d):
    return a * x + b * x ** 2 + c * x ** 3 + d


def _mos_restated(df_dist):
    popt, _ = curve_fit(_order_three, df_dist["Distance"].values, df_dist["mos"].values)
    dmap = df_dist["Distance"].apply(lambda x: _order_three(x, *popt))
    return dict(popt=popt, Distance_map=dmap, SRCC=spearmanr(df_dist["Distance"], df_dist["mos"])[0],
                SRCC_map=spearmanr(dmap, df_dist["mos"])[0], PCC=pearsonr(df_dist["Distance"], df_dist["mos"])[0],
                PCC_map=pearsonr(dmap, df_dist["mos"])[0])


def _same_mos(res, want):
    np.testing.assert_allclose(res["popt"], want["popt"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(res["table"]["Distance_map"].values, want["Distance_map"].values, rtol=1e-12, atol=1e-12)
    for k in ("SRCC", "SRCC_map", "PCC", "PCC_map"):
        assert abs(res[k] - want[k]) <= 1e-12, k


# ---- main ---------------------------------------------------------------------------------------------------------------------
def _yaml(tmp_path, **cfg):
    import yaml
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    return path


def test_main_rejects_an_unknown_experiment(tmp_path):
    with pytest.raises(SystemExit):
        T.main(["--config_file", _yaml(tmp_path, experiment_name="quality_xyz", checkpoint_path="seeded")])


@pytest.mark.parametrize("name", ["quality_nmr", "valid_rank", "intensity", "quality_fr"])
def test_main_dispatches_the_evaluation_experiments(tmp_path, name):
    """Without a GPU the call gets as far as the engine's own refusal - not the SystemExit these names used to end in."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        T.main(["--config_file", _yaml(tmp_path, experiment_name=name, checkpoint_path="seeded", nomad_model_path="seeded",
                                       eval_w2v=False)])


def test_experiment_names_are_the_reference_s():
    assert T.EVAL_EXPERIMENTS == ("quality_nmr", "valid_rank", "intensity", "quality_fr")
    for fn in ("eval_audio_quality", "eval_degr_level", "eval_degradation_intensity", "eval_full_reference", "get_embeddings_csv",
               "get_nmr_embeddings", "order_three", "euclidean_dist"):
        assert callable(getattr(T.Training, fn)), fn
    t = T.Training.__new__(T.Training)
    assert t.order_three(2.0, 1.0, 2.0, 3.0, 4.0) == 1 * 2 + 2 * 4 + 3 * 8 + 4
    a, b = np.array([1.0, 2.0, 3.0]), np.array([0.0, 4.0, 1.0])
    assert abs(t.euclidean_dist(a, b) - cdist(a[None], b[None])[0, 0]) < 1e-15


# ---- filters ------------------------------------------------------------------------------------------------------------------
def test_filters_by_db_and_conds(capsys):
    data = _database(np.random.default_rng(0))
    assert T.filter_test_data(data, None, None) is data
    got = T.filter_test_data(data, ["dbA", "dbC"], None)
    assert got.equals(data[data["db"].isin(["dbA", "dbC"])]) and set(got["db"]) == {"dbA", "dbC"}
    got = T.filter_test_data(data, ["dbB"], ["c1", "c4"])
    want = data[data["db"].isin(["dbB"])]
    want = want[want["condition"].str.contains("c1|c4")]
    assert got.equals(want) and set(got["condition"]) == {"dbB_c1", "dbB_c4"}
    assert "Testing DB: ['dbB'], conds: ['c1', 'c4']" in capsys.readouterr().out


# ---- quality_nmr --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [256, 768])
def test_quality_nmr_statistics(dim, capsys):
    rng = np.random.default_rng(1)
    data = _database(rng)
    ref = _emb_table([f"nmr/r{i}.wav" for i in range(5)], "reference", dim, rng).set_index("reference")
    for db_name, db in data.groupby("db"):
        level = [float(c.split("_c")[1]) for c in db["condition"]]
        df_emb = _emb_table(db["filepath_deg"], "filepath_deg", dim, rng, shift=0.3 * np.array(level))
        res = T.quality_nmr_stats(df_emb, db, ref, _nmr_mean)
        # train_triplet.py:262-280, restated
        test_embeddings = df_emb.set_index("filepath_deg")
        test_names = df_emb.merge(db, on="filepath_deg")[["filepath_deg", "condition", "mos"]]
        avg = np.mean(cdist(test_embeddings, ref), axis=1)
        df_dist = pd.DataFrame({"filepath_deg": test_embeddings.index, "Distance": avg})
        df_dist = df_dist.merge(test_names, on="filepath_deg").set_index("filepath_deg").groupby("condition").mean()
        assert list(res["table"].index) == list(df_dist.index) and len(df_dist) == 6
        np.testing.assert_allclose(res["table"]["Distance"].values, df_dist["Distance"].values, rtol=1e-13)
        np.testing.assert_allclose(res["table"]["mos"].values, df_dist["mos"].values, rtol=1e-15)
        _same_mos(res, _mos_restated(df_dist))
        assert res["embeddings"] is df_emb
    out = capsys.readouterr().out
    assert out.count("SRCC: ") == 3 and out.count("SRCC 3rd map: ") == 3 and out.count("PCC: ") == 3 and out.count("PCC 3rd map: ") == 3


# ---- quality_fr ---------------------------------------------------------------------------------------------------------------
def test_quality_fr_statistics():
    rng = np.random.default_rng(2)
    data = _database(rng)
    for db_name, db in data.groupby("db"):
        level = np.array([float(c.split("_c")[1]) for c in db["condition"]])
        df_ref = _emb_table(db["filepath_ref"], "filepath_ref", 256, rng)
        noise = rng.standard_normal((len(db), 256)).astype(np.float32) * (0.05 + 0.1 * level[:, None]).astype(np.float32)
        df_test = pd.concat([pd.DataFrame({"filepath_deg": list(db["filepath_deg"])}),
                             pd.DataFrame(df_ref.iloc[:, 1:].to_numpy(dtype=np.float32) + noise)], axis=1)
        res = T.quality_fr_stats(df_test, df_ref, db, _paired)
        # train_triplet.py:433-445, restated
        e_ref, e_test = df_ref.set_index("filepath_ref"), df_test.set_index("filepath_deg")
        test_names = df_test.merge(db, on="filepath_deg")[["filepath_deg", "condition", "mos"]]
        fr = np.diag(cdist(e_test, e_ref))
        df_dist = pd.DataFrame({"filepath_deg": e_test.index, "Distance": fr}).merge(test_names, on="filepath_deg")
        df_dist = df_dist.groupby("condition")[["Distance", "mos"]].mean()
        assert list(res["table"].index) == list(df_dist.index)
        np.testing.assert_allclose(res["table"]["Distance"].values, df_dist["Distance"].values, rtol=1e-13)
        _same_mos(res, _mos_restated(df_dist))
        assert abs(res["SRCC"] + 1.0) < 1e-12          # the noise grows with the level and MOS falls with it


# ---- intensity ----------------------------------------------------------------------------------------------------------------
def test_intensity_statistics(capsys):
    rng = np.random.default_rng(4)
    ref = _emb_table([f"nmr/r{i}.wav" for i in range(7)], "reference", 256, rng).set_index("reference")
    rows = [dict(Degradation=d, Condition=c, filepath_deg=f"mono/{d}_{c}_{f}.wav") for d in ("clip", "noise") for c in range(1, 6)
            for f in range(3)]
    data = pd.DataFrame(rows).sample(frac=1.0, random_state=5).reset_index(drop=True)
    for deg_name, deg_data in data.groupby("Degradation"):
        df_emb = _emb_table(deg_data["filepath_deg"], "filepath_deg", 256, rng, shift=0.2 * deg_data["Condition"].to_numpy())
        res = T.intensity_stats(df_emb, deg_data, ref, _nmr_mean, deg_name)
        # train_triplet.py:371-390, restated
        test_embeddings = df_emb.set_index("filepath_deg")
        test_names = df_emb.merge(deg_data, on="filepath_deg")[["filepath_deg", "Condition"]]
        avg = np.mean(cdist(test_embeddings, ref), axis=1)
        df_dist = pd.DataFrame({"filepath_deg": test_embeddings.index, "Distance": avg}).merge(test_names, on="filepath_deg")
        df_dist.set_index("filepath_deg", inplace=True)
        df_dist = df_dist.groupby("Condition").mean().reset_index()
        df_dist.sort_values(by="Distance", inplace=True)
        assert list(res["table"]["Condition"]) == list(df_dist["Condition"])
        np.testing.assert_allclose(res["table"]["Distance"].values, df_dist["Distance"].values, rtol=1e-13)
        assert abs(res["SRCC"] - spearmanr(df_dist["Distance"], df_dist["Condition"])[0]) <= 1e-12
    out = capsys.readouterr().out
    assert "Degradation: clip" in out and "Degradation: noise" in out and out.count("SRCC: ") == 2


# ---- valid_rank ---------------------------------------------------------------------------------------------------------------
def test_valid_rank_labels_and_statistics():
    anchors = ["/valid/spk1_noise_3.wav", "/valid/spk1_clip_1.wav", "/valid/spk2_noise_3.wav", "/valid/spk2_mp3_12.flac",
               "/valid/spk3_clip_1.wav", "/valid/spk9_clean_0.wav"]
    assert T.valid_rank_labels(anchors) == [x.split("_")[1] + " " + x.split("_")[2].split(".")[0] for x in anchors]
    assert T.valid_rank_labels(anchors)[:4] == ["noise 3", "clip 1", "noise 3", "mp3 12"]
    rng = np.random.default_rng(6)
    df_emb = _emb_table(anchors, "Anchor", 256, rng, shift=[3.0, 1.0, 2.8, 2.0, 1.1, 0.0])
    ref = _emb_table([f"nmr/r{i}.wav" for i in range(4)], "reference", 256, rng)
    res = T.valid_rank_stats(df_emb, ref, _nmr_mean)
    # train_triplet.py:317-333, restated
    avg = np.mean(cdist(df_emb.iloc[:, 1:].to_numpy(), ref.iloc[:, 1:].to_numpy()), axis=1)
    df_dist = pd.DataFrame({"Anchor": df_emb["Anchor"], "Distance": avg})
    df_dist.sort_values(by="Distance", inplace=True)
    df_dist["condition"] = [x.split("_")[1] + " " + x.split("_")[2].split(".")[0] for x in df_dist["Anchor"]]
    order = df_dist.groupby("condition")["Distance"].mean().sort_values().index
    assert list(res["table"]["Anchor"]) == list(df_dist["Anchor"]) and list(res["table"]["condition"]) == list(df_dist["condition"])
    np.testing.assert_allclose(res["table"]["Distance"].values, df_dist["Distance"].values, rtol=1e-13)
    assert res["order"] == list(order) and res["order"][0] == "clean 0"


def test_figures_are_written_with_matplotlib_alone(tmp_path):
    pytest.importorskip("matplotlib")
    rng = np.random.default_rng(7)
    df = pd.DataFrame({"mos": np.linspace(1.5, 4.5, 6), "Distance_map": np.linspace(4.4, 1.6, 6)})
    p = T.save_mos_scatter(df, str(tmp_path / "db_embeddings.png"), "Dist w.r.t. clean embeddings")
    assert p and os.path.getsize(p) > 1000
    box = pd.DataFrame({"condition": ["a 1"] * 4 + ["b 2"] * 4, "Distance": rng.random(8)})
    p = T.save_rank_boxplot(box, ["a 1", "b 2"], str(tmp_path / "validset_embeddings.png"))
    assert p and os.path.getsize(p) > 1000
    import sys
    assert "seaborn" not in sys.modules


# ---- Nomad.get_embeddings_csv with an Origw2v model (fake engine: tests/test_host.py's _FakeEngine, restated) --------------------
class _FakeEngine:
    """Records what the pipeline asks of an Engine; "embeds" a clip as [length, first sample, 0, ...]."""

    def __init__(self):
        self.calls = []

    def pack_ragged_host(self, waves):
        lens = [int(w.shape[0]) for w in waves]
        host = np.zeros((len(waves), max(lens)), dtype=np.float32)
        for i, w in enumerate(waves):
            host[i, :lens[i]] = w
        return host, lens

    def _embed(self, what, width, packed):
        host, lens = packed
        self.calls.append((what, list(lens)))
        out = np.zeros((len(lens), width), dtype=np.float32)
        out[:, 0] = lens
        out[:, 1] = host[:, 0]
        out[:, width - 1] = width
        return out

    def embed_ragged(self, waves, precision=None, packed=None):
        assert waves is None
        return self._embed("embed_ragged", 256, packed)

    def embed_features_ragged(self, waves, precision=None, packed=None):
        assert waves is None
        return self._embed("embed_features_ragged", 768, packed)

    def fetch_async(self, emb):
        class F:
            def result(self_inner):
                return emb
        return F()


def test_get_embeddings_csv_takes_the_model_it_is_given():
    from nomad_amd.nomad import Nomad, Origw2v, TripletModel
    import nomad_amd
    assert nomad_amd.Origw2v is Origw2v and "Origw2v" in nomad_amd.__all__
    lens = [300, 1200, 50, 700, 4000, 90]
    paths = [f"f{i}.wav" for i in range(len(lens))]
    eng = _FakeEngine()
    n = Nomad.__new__(Nomad)            # no GPU: only the host pipeline is under test
    n.engine, n.precision = eng, "fp32"

    def load(p, trim=False):
        i = int(os.path.basename(p)[1:-4])
        return np.full((1, lens[i]), float(i), dtype=np.float32)
    n.load_processing = load
    names = pd.DataFrame({"filename": paths})
    for model, width, call in ((Origw2v(eng), 768, "embed_features_ragged"), (TripletModel(eng), 256, "embed_ragged"),
                               (None, 256, "embed_ragged"), ("anything", 256, "embed_ragged")):
        eng.calls.clear()
        df = n.get_embeddings_csv(model, names, max_batch_samples=2000)
        assert df.shape == (len(lens), 1 + width), (model, df.shape)
        assert list(df["filename"]) == paths
        assert [int(x) for x in df[0]] == lens and [int(x) for x in df[1]] == list(range(len(lens)))
        assert (df[width - 1] == width).all()
        assert {c[0] for c in eng.calls} == {call} and [l for c in eng.calls for l in c[1]] == lens
    series = n.get_embeddings_csv(Origw2v(eng), names["filename"], root="root")     # a Series with a root, as the experiments call it
    assert series.shape == (len(lens), 769) and list(series["filename"]) == paths
