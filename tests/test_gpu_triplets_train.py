"""GPU: ``Nomad.mine_triplets`` - from clean clips to (Anchor, Positive, Negative) batches on the device - and one ``Training``
step with the config key ``triplets_on_device``.

* two clean clips of 0.5 s and 0.7 s, four conditions (noise at 20 and 5 dB SNR, clip factors 10 and 40), normalised to -23 LUFS:
  the NSIM table is ``Nomad.nsim``'s of the normalised rows against the un-normalised clips, and every gathered A / P / N row has
  the bytes of the row the index table names, rebuilt here with ``degrade`` and ``normalize`` called one by one;
* the loss of one optimisation step that ``Training.train()`` takes over a mined batch has the bits of ``train_step`` called by
  hand, on a second ``Training`` over the same seeded weights, with the (rows, lengths) pairs the miner gathered;
* the key with ``pad_mode: batch`` is a config error, raised before any GPU state exists."""
import struct

import numpy as np
import pytest
import torch

import nsim_ref as N

pytestmark = pytest.mark.gpu

LENS = [8000, 11200]
SNR, CLIP = [20.0, 5.0], [10.0, 40.0]
NO_REG = dict(dropout=0.0, attention_dropout=0.0, dropout_input=0.0, encoder_layerdrop=0.0)


def _speechlike(n, seed):
    """Noise under a slow envelope, 16-bit PCM: levels that the loudness gate passes and the clipper bites."""
    rng = np.random.RandomState(seed)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0 + seed)
    return (np.round(np.clip(0.2 * env * rng.randn(n), -1, 1) * 32767) / 32768.0).astype(np.float32)


def _write_wav(path, x, sr=16000):
    pcm = np.round(np.clip(x, -1, 1) * 32768.0).clip(-32768, 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" +
                struct.pack("<I", len(pcm)) + pcm)


def _bytes_equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def test_mined_rows_have_the_bytes_of_the_rows_the_table_names(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    clean = torch.zeros(2, max(LENS))
    for b, n in enumerate(LENS):
        clean[b, :n] = torch.from_numpy(_speechlike(n, 3 + b))
    noise = torch.from_numpy(N.pcm_noise(5000, 9, 0.2))
    A, P, Ng, info = nomad.mine_triplets(clean, noise=noise, snr_db=SNR, clip_factor=CLIP, normalize=-23.0, lengths=LENS, N=3,
                                         hard_sampling=False, margin=0.05, seed=4)
    t = info["triplets"]
    K = len(t["clip"])
    assert info["nsim"].shape == (2, 4) and info["conditions"] == [("noise", 20.0), ("noise", 5.0), ("clip", 10.0), ("clip", 40.0)]
    assert 1 <= K <= 6 and K + info["dropped"] == 6, (K, info["dropped"])
    print("NSIM table", info["nsim"].tolist(), "rows", K, "dropped", info["dropped"])
    # the table: Nomad.nsim of the normalised rows against the un-normalised clips
    members = []
    for kind, levels in (("noise", SNR), ("clip", CLIP)):
        rows, lens_rep = nomad.degrade(clean, kind, levels, noise=noise if kind == "noise" else None, lengths=LENS)
        rows, lens_rep, _ = nomad.normalize(rows, lengths=lens_rep)
        score = nomad.nsim((rows, lens_rep), clean, lengths=LENS).cpu().numpy()
        at = 0 if kind == "noise" else 2
        assert np.array_equal(score.view(np.uint64), np.ascontiguousarray(info["nsim"][:, at:at + 2]).view(np.uint64)), kind
        members.append(rows.view(2, 2, -1))
    members.append(nomad.normalize(clean, lengths=LENS)[0].view(2, 1, -1))
    bank = torch.cat(members, dim=1)                               # (clip, member, stride): member 4 is the clean clip
    assert (info["nsim"][:, 0] > info["nsim"][:, 1]).all() and (info["nsim"][:, 2] > info["nsim"][:, 3]).all() and (info["nsim"] < 1).all()
    for (rows, lens), key in ((A, "anchor"), (P, "positive"), (Ng, "negative")):
        assert rows.shape == (K, bank.shape[2]) and rows.dtype == torch.float32 and rows.is_cuda and lens == [LENS[b] for b in t["clip"]]
        for i in range(K):
            want = bank[int(t["clip"][i]), int(t[key][i])]
            assert _bytes_equal(rows[i], want), (key, i, int(t["clip"][i]), int(t[key][i]))
            assert not rows[i, lens[i]:].any(), "zero behind the length"
    assert (t["anc_pos_dist"] < t["anc_neg_dist"]).all() and (t["anc_neg_dist"] > t["anc_pos_dist"] + 0.05).all()
    again = nomad.mine_triplets(clean, noise=noise, snr_db=SNR, clip_factor=CLIP, normalize=-23.0, lengths=LENS, N=3, seed=4)
    assert all(_bytes_equal(x[0], y[0]) for x, y in zip((A, P, Ng), again[:3])), "the same seed gives the same batch"
    # without normalisation the members are the degraded rows as they are, and the clean member is the clip
    A2, _, _, info2 = nomad.mine_triplets(clean, clip_factor=CLIP + [80.0], normalize=None, lengths=LENS, N=1, hard_sampling=True, seed=1)
    rows, _ = nomad.degrade(clean, "clip", CLIP + [80.0], lengths=LENS)
    bank2 = torch.cat([rows.view(2, 3, -1), clean.to(rows.device).view(2, 1, -1)], dim=1)
    t2 = info2["triplets"]
    for i in range(len(t2["clip"])):
        assert _bytes_equal(A2[0][i], bank2[int(t2["clip"][i]), int(t2["anchor"][i])])
    with pytest.raises(ValueError, match="needs snr_db, clip_factor or reverberance"):
        nomad.mine_triplets(clean, lengths=LENS)
    with pytest.raises(ValueError, match="noise"):
        nomad.mine_triplets(clean, snr_db=SNR, lengths=LENS)


def _config(tmp_path, **over):
    clean_dir, valid_dir = tmp_path / "clean", tmp_path / "valid"
    clean_dir.mkdir(exist_ok=True)
    valid_dir.mkdir(exist_ok=True)
    for b, n in enumerate(LENS):
        _write_wav(str(clean_dir / f"clip{b}.wav"), _speechlike(n, 3 + b))
        _write_wav(str(valid_dir / f"clip{b}.wav"), _speechlike(n, 13 + b))
    _write_wav(str(tmp_path / "noise.wav"), N.pcm_noise(5000, 9, 0.2))
    cfg = dict(experiment_name="Training", out_dir="toy", training_script="src.training.train_triplet", root=str(tmp_path),
               train_df="unused.csv", valid_df="unused.csv", sampling_rate=16000, train_bs=6, val_bs=6, test_bs=1, lr=1e-4,
               lr_decay_factor=0.5, lr_decay_step=1, num_epochs=1, num_workers=0, emb_dim=256, patience=200, checkpoint_path="seeded",
               ssl_out_dim=768, margin=0.2, freeze_convnet=True, freeze_all=False, trim=False, eval_w2v=False, pad_mode="exact",
               triplets_on_device=dict(clean=str(clean_dir), valid_clean=str(valid_dir), noise=str(tmp_path / "noise.wav"), snr_db=SNR,
                                       clip=CLIP, normalize=-23, N=3, hard_sampling=False, sampling_margin=0.05))
    cfg.update(over)
    return cfg


def test_the_key_with_pad_mode_batch_is_a_config_error(tmp_path):
    from nomad_amd.train import Training
    with pytest.raises(ValueError, match="requires pad_mode: exact"):
        Training(_config(tmp_path, pad_mode="batch"))
    with pytest.raises(ValueError, match="unknown keys"):
        Training(_config(tmp_path, triplets_on_device=dict(clean="a", valid_clean="b", clip=[10], snr=[5])))


def test_one_training_step_on_mined_triplets_has_the_bits_of_the_step_by_hand(tmp_path):
    from nomad_amd.train import MinedTriplets, Training
    cfg = _config(tmp_path)
    tr = Training(cfg, regularisation=NO_REG)
    try:
        assert isinstance(tr.train_loader, MinedTriplets) and len(tr.train_loader) == 1 and not hasattr(tr, "train_set")
        valid = [tr.eval(), tr.eval()]
        assert np.isfinite(valid[0]) and valid[0] == valid[1], "validation mines with a fixed seed: successive epochs are comparable"
        before = tr.engine.train_read(0).clone()
        loss_loop = tr.train()                                     # one batch: one optimisation step
        assert np.isfinite(loss_loop) and not torch.equal(before, tr.engine.train_read(0)), "the step moved the weights"
        mined = tr.train_loader.last_info
    finally:
        tr.engine.close()
    hand = Training(cfg, regularisation=NO_REG)
    try:
        A, P, Ng = next(iter(hand.train_loader))
        t, want = hand.train_loader.last_info["triplets"], mined["triplets"]
        assert all(np.array_equal(t[k], want[k]) for k in want) and 1 <= len(A[1]) <= 6
        assert A[0].shape == P[0].shape == Ng[0].shape and A[0].is_cuda
        loss_hand = hand.train_step(A, P, Ng)
        print("loss of the loop's step", loss_loop, "by hand", loss_hand.item(), "triplets", len(A[1]))
        assert np.float32(loss_loop).view(np.uint32) == np.float32(loss_hand.item()).view(np.uint32)
    finally:
        hand.engine.close()
