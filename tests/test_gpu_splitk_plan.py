"""GPU: WHICH path a loss-path call took - the split-K GEMMs and their fused epilogues - read off the profiling regions.

The other split-K tests compare values (fused against unfused bit for bit, both sides of a switch against float64) and would pass
if no GEMM split and no epilogue fused.  Here the regions of one call are counted per kernel class (Engine.profile_read: one
region per Scope, not per launch).  A split GEMM is one GEMM-class region (its slices) plus one row-op region (its epilogue); a
stand-alone LayerNorm, or LayerNorm backward, is one row-op region; a fusion removes one."""
import pytest
import torch

from nomad_amd.weights import num_frames

pytestmark = pytest.mark.gpu

CLASSES = ("gemm_mfma_all", "attention_mfma", "rowwise")


def _wav(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(B, n, generator=g)).cuda()


def _regions(eng, call):
    """-> (what `call` returned, {kernel class: regions it opened})."""
    eng.profile_reset()
    out = call()
    torch.cuda.synchronize()
    table = eng.profile_read()
    return out, {k: table[k]["launches"] for k in CLASSES}


def test_fused_split_k_epilogues_run(built_lib, sd0, monkeypatch):
    """(2, 8000): T = 24, M = 48 - every transformer GEMM of the training-mode forward and the dX-only backward is on the 64 x 64
    tile and splits K.  NOMAD_SPLITK_LN=1 takes 24 row-op regions out of the forward (the LayerNorm behind out_proj and fc2 of each
    of 12 layers runs in the GEMM's epilogue), NOMAD_SPLITK_LNB=1 takes 24 out of the backward (the LayerNorm backward behind 12
    fc1^T, behind the 11 qkv^T in front of the LN2 of the layer below, behind the 1 in front of the encoder LayerNorm).  GEMM and
    attention regions do not move, and every output is the same bits."""
    from nomad_amd.engine import Engine
    n = 8000
    assert num_frames(n) == 24
    wav = _wav(2, n, 11)
    runs = {}
    for var in ("NOMAD_SPLITK_LN", "NOMAD_SPLITK_LNB"):
        for flag in ("0", "1"):
            monkeypatch.setenv(var, flag)
            eng = Engine(sd0, 0, diag=True)
            eng.profile_enable()
            (emb, layers, saved), fwd = _regions(eng, lambda: eng.embed_train(wav))
            g2 = torch.Generator().manual_seed(12)
            dl = (torch.randn(layers.shape, generator=g2) / layers.numel()).cuda()
            de = (torch.randn(emb.shape, generator=g2) / emb.numel()).cuda()
            dwav, bwd = _regions(eng, lambda: eng.embed_backward(wav, layers, saved, dl, de))
            runs[var, flag] = (fwd, bwd, (emb.clone(), layers.clone(), dwav.clone()))
            eng.close()
            print(var, flag, "forward", fwd, "backward", bwd)
        monkeypatch.delenv(var)
    for var, fused_pass, other_pass in (("NOMAD_SPLITK_LN", 0, 1), ("NOMAD_SPLITK_LNB", 1, 0)):
        off, on = runs[var, "0"], runs[var, "1"]
        assert off[fused_pass]["rowwise"] - on[fused_pass]["rowwise"] == 24, var
        assert off[other_pass]["rowwise"] == on[other_pass]["rowwise"], var
        for p in (0, 1):
            assert off[p]["gemm_mfma_all"] == on[p]["gemm_mfma_all"] and off[p]["attention_mfma"] == on[p]["attention_mfma"], var
        assert torch.isfinite(on[2][2]).all() and on[2][2].abs().max() > 0
        for a, b in zip(off[2], on[2]):
            assert torch.equal(a, b), var
    # both switches at their default (on) in the second run of each pair: the same call, the same regions
    assert runs["NOMAD_SPLITK_LN", "1"][:2] == runs["NOMAD_SPLITK_LNB", "1"][:2]


def test_what_splits_is_a_function_of_shape_and_kind_of_call(engine):
    """(5, 41040): M = 640, fc1's 64 x 64 tiles number 480 < 512; (5, 41360): M = 645, 528 tiles (the fc1 pair of
    test_gpu_backward_f64.py's switch table; its GELU keeps it out of both fusions).  Every other GEMM decides the same on both
    sides.  The no-gradient layer-output forward opens exactly 12 row-op regions more at M = 640: fc1's epilogue in 12 layers.  The
    training-mode forward opens the SAME number on both sides: there fc1 also writes its pre-activation for the backward (Upre),
    which keeps it off split-K at any M - so embed_train is held to its own switch, the qkv pair of that table, (4, 71760) |
    (4, 72080): M = 896 | 900, 504 | 540 tiles, 12 regions.  A call that may not split (scoring forward, ragged batch) opens the
    same number on both sides of either switch.  The counts are the parent commit's (profiles/NOTEBOOK.md)."""
    g = torch.Generator().manual_seed(13)
    head = ((0.02 * torch.randn(256, 768, generator=g)).cuda(), (0.02 * torch.randn(256, generator=g)).cuda())
    calls = {
        "embed_train": lambda w, B, n: engine.embed_train(w),
        "embed layers": lambda w, B, n: engine.embed(w, head=head, want_layers=True),
        "embed scoring": lambda w, B, n: engine.embed(w),
        "embed_train_ragged": lambda w, B, n: engine.embed_train_ragged(w, lengths=[n] * B),
    }
    # (B, samples below, samples above, frames below, frames above, {call: row-op regions more below the switch})
    switches = ((5, 41040, 41360, 128, 129, {"embed_train": 0, "embed layers": 12, "embed scoring": 0, "embed_train_ragged": 0}),
                (4, 71760, 72080, 224, 225, {"embed_train": 12, "embed layers": 12, "embed scoring": 0, "embed_train_ragged": 0}))
    rows = {}
    engine.profile_enable()
    try:
        for B, below, above, t_below, t_above, _ in switches:
            assert (num_frames(below), num_frames(above)) == (t_below, t_above)
            for n in (below, above):
                wav = _wav(B, n, n)
                for name, call in calls.items():
                    _, rows[name, n] = _regions(engine, lambda: call(wav, B, n))
                    print(name, (B, n), rows[name, n])
    finally:
        engine.profile_enable(False)
    for B, below, above, _, _, extra in switches:
        for name, more in extra.items():
            assert rows[name, below]["rowwise"] - rows[name, above]["rowwise"] == more, (name, B, below)
            assert rows[name, below]["gemm_mfma_all"] == rows[name, above]["gemm_mfma_all"], (name, B, below)
