"""Host side of the layer-weighted / per-utterance NOMAD loss: ``loss_selection`` maps (``NomadLoss.L``, ``layer_weights``) to
the 13 weights of the terms and the encoder depth they need, ``check_reduction`` validates the reduction.  No GPU."""
import math

import pytest

from nomad_amd.nomad import check_reduction, loss_selection


@pytest.mark.parametrize("L,depth", [(1, 1), (6, 6), (12, 12), (13, 12)])
def test_L_maps_to_the_first_L_terms(L, depth):
    weights, d = loss_selection(L)
    assert weights == [1.0] * L + [0.0] * (13 - L) and len(weights) == 13
    assert d == depth


def test_depth_is_one_past_the_deepest_weighted_layer():
    w = [0, 0, 0, 1, 0, 0, 0, 0, 0, 2.5, 0, 0, 0]
    weights, depth = loss_selection(13, w)       # explicit weights win over L
    assert weights == [float(x) for x in w] and depth == 10
    assert loss_selection(3, w) == (weights, 10)
    assert loss_selection(13, [1] + [0] * 12)[1] == 1


def test_an_embedding_weight_needs_the_whole_encoder():
    assert loss_selection(13, [0] * 12 + [1])[1] == 12
    assert loss_selection(13, [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.25])[1] == 12
    assert loss_selection(13, [1.0] * 13) == ([1.0] * 13, 12)


@pytest.mark.parametrize("L", [0, 14, -1, 6.0, "6", None, True])
def test_bad_L_is_rejected(L):
    with pytest.raises(ValueError):
        loss_selection(L)


@pytest.mark.parametrize("w", [[1.0] * 12, [1.0] * 14, [1.0] * 12 + [-0.5], [-1e-9] + [1.0] * 12, [math.nan] + [1.0] * 12,
                               [math.inf] + [1.0] * 12, [0.0] * 13, []],
                         ids=["12", "14", "negative-emb", "negative-layer", "nan", "inf", "all-zero", "empty"])
def test_bad_weights_are_rejected(w):
    with pytest.raises(ValueError):
        loss_selection(13, w)


def test_weights_may_be_a_tensor():
    import torch
    weights, depth = loss_selection(13, torch.tensor([0.5] * 4 + [0.0] * 9))
    assert weights == [0.5] * 4 + [0.0] * 9 and depth == 4


def test_reduction():
    assert check_reduction("mean") == "mean" and check_reduction("none") == "none"
    for bad in ("sum", "None", None, 0, ""):
        with pytest.raises(ValueError):
            check_reduction(bad)
