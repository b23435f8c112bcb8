"""CPU: the host side of exact-length (ragged) training and loss - the collate that keeps lengths, ``pad_mode`` validation and
the argument checks of ``Nomad.forward(estimate, clean, lengths)``.  Nothing here touches a GPU."""
import numpy as np
import pytest
import torch


def _wavs(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, n, generator=g) for n in lens)


def test_collate_exact_keeps_lengths_and_one_storage_width():
    from nomad_amd.train import TripletDataset
    A, P, N = _wavs([5000, 7001], 0), _wavs([6100, 5003], 1), _wavs([9000, 4000], 2)
    (a, la), (p, lp), (n, ln) = TripletDataset.collate_exact(A, P, N)
    assert a.shape == p.shape == n.shape == (2, 1, 9000)
    assert la.tolist() == [5000, 7001] and lp.tolist() == [6100, 5003] and ln.tolist() == [9000, 4000]
    assert la.dtype == torch.int32
    for rows, lens, src in ((a, la, A), (p, lp, P), (n, ln, N)):
        for i, w in enumerate(src):
            assert torch.equal(rows[i, 0, :lens[i]], w[0])
            assert not rows[i, 0, lens[i]:].any()


def test_collate_fn_follows_pad_mode():
    from nomad_amd.train import TripletDataset
    ds = TripletDataset.__new__(TripletDataset)      # (no csv needed for the collate)
    batch = list(zip(_wavs([5000, 7001], 0), _wavs([6100, 5003], 1), _wavs([9000, 4000], 2)))
    ds.pad_mode = "batch"
    a, p, n = ds.collate_fn(batch)                   # the reference's collate: each branch to its own maximum
    assert a.shape == (2, 1, 7001) and p.shape == (2, 1, 6100) and n.shape == (2, 1, 9000)
    ref = TripletDataset.zero_pad_wav([b[0] for b in batch])
    assert torch.equal(a, ref)
    ds.pad_mode = "exact"
    (a, la), _, _ = ds.collate_fn(batch)
    assert a.shape == (2, 1, 9000) and la.tolist() == [5000, 7001]
    del ds.pad_mode                                  # an object made before the key existed behaves like "batch"
    assert torch.equal(ds.collate_fn(batch)[0], ref)


def test_pad_mode_validation():
    from nomad_amd.train import PAD_MODES, check_pad_mode
    assert PAD_MODES == ("batch", "exact")
    assert check_pad_mode({}) == "batch"
    assert check_pad_mode({"pad_mode": "exact"}) == "exact"
    assert check_pad_mode({"pad_mode": "exact", "freeze_convnet": True}) == "exact"
    assert check_pad_mode({"pad_mode": "exact", "freeze_convnet": False, "freeze_all": True}) == "exact"   # freeze_all freezes it again
    assert check_pad_mode({"pad_mode": "batch", "freeze_convnet": False}) == "batch"
    with pytest.raises(ValueError, match="freeze_convnet: True"):
        check_pad_mode({"pad_mode": "exact", "freeze_convnet": False})
    with pytest.raises(ValueError, match="pad_mode must be one of"):
        check_pad_mode({"pad_mode": "max"})


def test_training_refuses_a_bad_pad_mode_before_it_needs_a_gpu():
    """A config error is a ValueError at construction, ahead of the "no CPU path" error of a host without a GPU."""
    from nomad_amd.train import Training
    cfg = dict(experiment_name="Training", checkpoint_path="seeded", margin=0.2)
    with pytest.raises(ValueError, match="pad_mode must be one of"):
        Training(dict(cfg, pad_mode="longest"))
    with pytest.raises(ValueError, match="freeze_convnet: True"):
        Training(dict(cfg, pad_mode="exact", freeze_convnet=False))


def test_ragged_metadata_is_the_plain_prefix_sums(built_lib):
    """nomad_ragged_metadata: the ints every ragged entry point copies ahead of its kernels, restated in plain Python -
    [lens | pref_0..6 | ppref | bpref | pairpref_1..4 | upref_0..6 | epref_0..3 | opref_0..3], B + 1 ints per prefix array; the
    backward's three groups: upref_i[c] = pref_i[c] + 2 c (padded dU rows), epref_i / opref_i = prefix sums of ceil(L_i / 2) /
    floor(L_i / 2).  Lengths with T = 1, 2, 64, 65, 130 and odd and even L_i at every level."""
    import ctypes as C
    from nomad_amd import _lib
    lib = _lib.load()
    lens = [400, 870, 20671, 21050, 41685, 11237, 160000]
    B = len(lens)

    def conv_lens(n):
        out = []
        for k, s in zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)):
            n = (n - k) // s + 1
            out.append(n)
        return out

    L = [conv_lens(n) for n in lens]
    assert [l[6] for l in L][:5] == [1, 2, 64, 65, 130]
    for i in range(7):
        assert {l[i] % 2 for l in L} == {0, 1}, i
    arr, n = (C.c_int * B)(*lens), C.c_size_t()
    assert lib.nomad_ragged_metadata(B, arr, None, 0, C.byref(n)) == 0
    assert n.value == B + 28 * (B + 1)
    out = (C.c_int * n.value)()
    assert lib.nomad_ragged_metadata(B, arr, out, n.value - 1, C.byref(n)) == _lib.NOMAD_ERR_WORKSPACE
    assert lib.nomad_ragged_metadata(B, arr, out, n.value, C.byref(n)) == 0
    meta = np.array(out[:])
    pre = lambda xs: np.concatenate([[0], np.cumsum(xs)])
    off = lambda k: B + k * (B + 1)
    blk = lambda k: meta[off(k):off(k + 1)]
    assert np.array_equal(meta[:B], lens)
    for i in range(7):
        assert np.array_equal(blk(i), pre([l[i] for l in L])), i
        assert np.array_equal(blk(13 + i), pre([l[i] + 2 for l in L])), i
        assert np.array_equal(blk(13 + i), blk(i) + 2 * np.arange(B + 1)), i
    assert np.array_equal(blk(7), pre([l[6] + 128 for l in L]))
    for i in range(1, 5):
        assert np.array_equal(blk(8 + i), pre([(l[i] + 1) // 2 for l in L])), i
    for i in range(4):
        assert np.array_equal(blk(20 + i), pre([(l[i] + 1) // 2 for l in L])), i
        assert np.array_equal(blk(24 + i), pre([l[i] // 2 for l in L])), i
        assert np.array_equal(blk(20 + i) + blk(24 + i), blk(i)), i
    bad = (C.c_int * B)(*([399] + lens[1:]))
    assert lib.nomad_ragged_metadata(B, bad, None, 0, C.byref(n)) == _lib.NOMAD_ERR_INVALID


def test_check_lengths():
    from nomad_amd.nomad import MIN_SAMPLES, check_lengths
    w = torch.zeros(3, 1, 8000)
    assert check_lengths(w, [400, 8000, 5000]) == [400, 8000, 5000]
    assert check_lengths(w.squeeze(1), torch.tensor([400, 8000, 5000])) == [400, 8000, 5000]
    assert check_lengths(w, np.array([400, 8000, 5000]).tolist()) == [400, 8000, 5000]
    assert MIN_SAMPLES == 400
    with pytest.raises(ValueError, match="entries for a batch of 3"):
        check_lengths(w, [400, 8000])
    with pytest.raises(ValueError, match=r"lengths\[1\] = 8001"):
        check_lengths(w, [400, 8001, 5000])
    with pytest.raises(ValueError, match=r"lengths\[0\] = 399"):
        check_lengths(w, [399, 8000, 5000])
    with pytest.raises(ValueError, match="1-D integer tensor"):
        check_lengths(w, torch.tensor([400.0, 8000.0, 5000.0]))
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        check_lengths(torch.zeros(3, 2, 8000), [400, 8000, 5000])
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        check_lengths(torch.zeros(8000), [400])


def test_nomad_forward_checks_its_lengths_before_it_touches_the_engine():
    """``Nomad.forward`` and ``graphed_loss`` on an object without an engine: the argument checks come first."""
    from nomad_amd.nomad import Nomad
    nmd = Nomad.__new__(Nomad)
    e, c = torch.zeros(2, 1, 8000), torch.zeros(2, 1, 8000)
    with pytest.raises(ValueError, match="must have one shape"):
        nmd.forward(e, torch.zeros(2, 1, 8001), lengths=[8000, 8000])
    with pytest.raises(ValueError, match=r"lengths\[1\] = 9000"):
        nmd.forward(e, c, lengths=[8000, 9000])
    with pytest.raises(ValueError, match="entries for a batch of 2"):
        nmd.forward(e, c, lengths=[8000])
    with pytest.raises(ValueError, match="ONE batch shape"):
        nmd.graphed_loss(e, c, lengths=[8000, 8000])


def test_binding_declares_the_ragged_gradient_entry_points():
    from nomad_amd import _lib
    for name in ("nomad_saved_bytes_ragged", "nomad_backward_workspace_bytes_ragged", "nomad_train_workspace_bytes_ragged",
                 "nomad_embed_train_ragged", "nomad_embed_backward_ragged", "nomad_train_backward_ragged", "nomad_l1_loss_ragged",
                 "nomad_l1_loss_backward_ragged", "nomad_ragged_metadata"):
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 3
