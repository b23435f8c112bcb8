"""Float64 references with an fp32 yardstick, for the backward and training tests (``test_gpu_backward_f64.py``,
``test_gpu_train_f64.py``, ``test_gpu_train_mode_f64.py``).  Imported by the tests like ``conftest``; not a test module itself.

Method (the one ``test_gpu_kernels.py``'s attention test uses for the forward): the same CPU computation - the oracle
(``oracle/nomad_oracle.py``, unchanged) or plain ``torch.autograd`` - runs twice, once with every parameter and input in
float64 (the truth) and once in fp32.  Per tensor,

    e32     = max |fp32 result - float64 result|      (what plain fp32 arithmetic gets on this problem)
    err_gpu = max |GPU result  - float64 result|

and the GPU must satisfy ``err_gpu <= C * e32 + FLOOR * top``, ``top`` = the largest |float64 value| over all tensors of
the case.  The floor only matters for tensors whose true value is (close to) zero: ``k_proj.bias``'s gradient is
exactly 0 (softmax is shift invariant), so both sides hold rounding noise of the other tensors' size.

C = 8 and FLOOR = 1e-7, for every case of both files.  Measured on one MI355X (err_gpu / e32, worst tensor per case):
attention backward at most 5.4 (7.2 with a forced late rescale), LayerNorm backward 1.4, the loss path's d loss / d waveform
1.5 - 2.5 (configs[4], 32 x 16384: 1.7), the training step's parameter gradients 5.0 - 5.8 (the reference shape,
3 x (8, 160000) merged: 5.4).  The fp32-oracle bounds of test_gpu_backward.py / test_gpu_train.py (1e-3 relative on dwav,
2e-4 of each gradient's max) sit two to three orders of magnitude above the fp32 error.

One stage has a wider yardstick, the attention backward (test_gpu_backward_f64._attention_case).  There e32 is, per tensor,
the larger fp32 error of two formulations - autograd's softmax backward (sum_j p_j dP_j) and the kernels' own (probabilities
exp(s - lse), row term D = rowsum(dctx * out)) - and dq / dk also take a first-order rounding bound of D.  Autograd's form
cancels exactly for a one-hot row (T = 1: e32 = 0 for dq / dk), the kernels' does not; how much error the kernels' form
shows on the CPU depends on the BLAS's summation order.  At small T it is up to ~3x autograd's, so against plain fp32
autograd alone the attention backward's effective constant is nearer 20 than 8.

test_gpu_train_mode_f64.py (train mode with the engine's masks, Adam, and - with test_gpu_forward_f64.C_X3P = 80 in front of
e32 - bf16x3 products on the gradient paths) measured: train-mode gradients 4.4 - 7.0, embeddings 2.2 - 3.5; bf16x3 training
gradients 26.9 - 39.4, its loss path 9.8 - 14.0; Adam's parameters and moments 1.00 (its docstring has the table).

The CPU threads are torch's default (``OMP_NUM_THREADS``)."""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import torch

from nomad_amd.weights import num_frames
from oracle import nomad_oracle as O

C = 8.0
FLOOR = 1e-7


def cast(x, dtype):
    """A tensor, a state dict or a tuple of either, in ``dtype`` (fp32 / float64); other values pass through."""
    if isinstance(x, torch.Tensor):
        return x.to(dtype) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: cast(v, dtype) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(cast(v, dtype) for v in x)
    return x


def both(fn: Callable, *args, **kw):
    """fn(*args) with every floating tensor in float64, then in fp32 -> (result64, result32)."""
    return fn(*cast(args, torch.float64), **kw), fn(*cast(args, torch.float32), **kw)


def as_dict(x) -> Dict[str, torch.Tensor]:
    if isinstance(x, dict):
        return x
    if isinstance(x, (tuple, list)):
        return {str(i): v for i, v in enumerate(x)}
    return {"": x}


def _maxabs(t: torch.Tensor) -> float:
    return t.abs().max().item() if t.numel() else 0.0


def measure(got, ref64, ref32, e32_min=None, c: float = C) -> Dict[str, Tuple[float, float, float]]:
    """{name: (err_gpu, e32, bound)} for a tensor, a tuple or a dict of tensors (the same structure in all three).
    e32_min: {name: a first-order rounding bound of fp32} for a stage whose fp32 reference happens to be exact where
    the kernel's formulation is not (the caller states why).  c: the constant in front of e32 (C unless the caller's
    module docstring gives a path its own)."""
    g, r, r32 = as_dict(got), as_dict(ref64), as_dict(ref32)
    top = max(_maxabs(v) for v in r.values())
    out = {}
    for k, want in r.items():
        want = want.detach().double()
        err = _maxabs(g[k].detach().cpu().double() - want)
        e32 = max(_maxabs(r32[k].detach().double() - want), (e32_min or {}).get(k, 0.0))
        out[k] = (err, e32, c * e32 + FLOOR * top)
    return out


def check(case: str, got, ref64, ref32, e32_min=None, c: float = C) -> Dict[str, Tuple[float, float, float]]:
    """Assert err_gpu <= c * e32 + FLOOR * top for every tensor; prints the worst tensor's err_gpu / e32 (the number the
    module docstring records) and its share of the bound."""
    res = measure(got, ref64, ref32, e32_min, c)
    worst = max(res, key=lambda k: res[k][0] / res[k][2] if res[k][2] > 0 else float("inf"))
    err, e32, bound = res[worst]
    ratio = err / e32 if e32 > 0 else float("inf")
    print(f"F64 {case}: worst '{worst}' err_gpu {err:.3e} e32 {e32:.3e} err_gpu/e32 {ratio:.2f} of_bound {err / bound:.3f}")
    bad = {k: v for k, v in res.items() if not v[0] <= v[2]}
    assert not bad, f"{case}: err_gpu > {c} e32 + {FLOOR} top for " + ", ".join(
        f"{k} ({v[0]:.3e} > {v[2]:.3e}, e32 {v[1]:.3e})" for k, v in sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][2])[:4])
    return res


def n_for(T: int) -> int:
    """The fewest samples per clip that give T frames (every conv layer then divides its input exactly)."""
    n = 320 * T
    while num_frames(n - 1) >= T:
        n -= 1
    while num_frames(n) < T:
        n += 1
    return n


# ---- oracle paths ---------------------------------------------------------------------------------------------------------
def lossnet_dwav(sd, wav, emb_w, emb_b, G_layers, G_emb, feature_grad_mult):
    """d <outputs, G> / d wav of ``LossNetLayers.forward`` (the loss path's 13 outputs) under the smooth functional
    sum_l <layer_l, G_layers[l]> + <emb, G_emb>, in the dtype of the arguments."""
    w = wav.clone().requires_grad_(True)
    outs = O.lossnet_forward(sd, w, emb_w, emb_b, feature_grad_mult=feature_grad_mult, required_seq_len_multiple=2)
    s = sum((outs[i] * G_layers[i]).sum() for i in range(12)) + (outs[12] * G_emb).sum()
    (grad,) = torch.autograd.grad(s, w)
    return grad


KINK = 1e-4


def head_relu_undecided(sd, wav):
    """Channels of the head's ReLU input (the time mean of the last layer, 768 per clip) that lie within KINK of zero for
    some clip, in float64.  There the derivative of the ReLU is decided by the forward's own rounding: the mean of one
    channel of test_gpu_backward_f64's (8, 336) case is 2.8e-7, half of the fp32 oracle's error on that mean (5.5e-7), and
    an engine with bf16x3 products, whose forward lands on the other side, differs from float64 there by 4 % of that clip's
    d emb / d waveform - no error of the backward.  The loss path's tests use a head of their own and zero its columns
    for these channels, so that neither side's result depends on them.  KINK = 1e-4 is the error test_gpu_forward_f64.py
    allows the least precise fp32-buffer mode on these values (C_X3P = 80 times an e32 of 1e-6); the means have an rms of
    0.9, so a handful of the 768 columns go."""
    with torch.no_grad():
        x, _ = O.backbone(cast(sd, torch.float64), wav.double(), required_seq_len_multiple=2)
    undecided = (x.mean(1).abs() < KINK).any(0)
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    return undecided


def triplet_grads(sd, A, P, N, margin, freeze_convnet=True, feature_grad_mult=0.1, stoch=None):
    """``O.triplet_step_grads`` in the dtype of the arguments -> (loss, {key: gradient}).  stoch: one ``O.Stochastic`` per
    branch (train mode), None = eval-mode arithmetic."""
    return O.triplet_step_grads(sd, A, P, N, margin, stoch, freeze_convnet=freeze_convnet, feature_grad_mult=feature_grad_mult)


def triplet_batch(B, T, seed):
    """Anchor, positive and negative clips, B each, of the fewest samples that give T frames: 0.1 * randn, clamped."""
    g = torch.Generator().manual_seed(seed)
    n = n_for(T)
    return [(0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1) for _ in range(3)]


def _live(sd, freeze_convnet):
    sd = {k: v.clone() for k, v in sd.items()}
    keys = O.trainable_keys(sd, freeze_convnet)
    for k in keys:
        sd[k].requires_grad_(True)
    return sd, keys


def triplet_step(sd, A, P, N, margin, stoch=None, freeze_convnet=True, feature_grad_mult=0.1):
    """The reference's three forward calls (one ``O.Stochastic`` per branch, None = eval-mode arithmetic), the triplet loss
    and its backward, in the dtype of the arguments -> (loss, embeddings (3B, 256) in the order A | P | N, {key: gradient}).
    ``O.triplet_step_grads`` with the embeddings kept."""
    st = list(stoch) if stoch is not None else [None, None, None]
    sd, keys = _live(sd, freeze_convnet)
    fgm = 1.0 if freeze_convnet else feature_grad_mult
    embs = [O.triplet_forward(sd, w, s, fgm) for w, s in zip((A, P, N), st)]
    loss = torch.nn.TripletMarginLoss(margin=margin)(*embs)
    grads = torch.autograd.grad(loss, [sd[k] for k in keys])
    return loss.detach(), torch.cat(embs).detach(), dict(zip(keys, grads))


def merged_triplet_step(sd, A, P, N, margin, stoch=None, freeze_convnet=True, feature_grad_mult=0.1):
    """The same step as ONE forward over the concatenated batch A | P | N with one ``O.Stochastic`` (one seed: the mask of an
    element depends on its index in the whole batch; ``branch_masks``: LayerDrop per branch), the loss on the three thirds.
    A layer that every branch drops gets a zero gradient.  -> (loss, embeddings (3B, 256), {key: gradient})."""
    B = A.shape[0]
    sd, keys = _live(sd, freeze_convnet)
    e = O.triplet_forward(sd, torch.cat([A, P, N]), stoch, 1.0 if freeze_convnet else feature_grad_mult)
    loss = torch.nn.TripletMarginLoss(margin=margin)(e[:B], e[B:2 * B], e[2 * B:])
    grads = torch.autograd.grad(loss, [sd[k] for k in keys], allow_unused=True)
    return loss.detach(), e.detach(), {k: (g if g is not None else torch.zeros_like(sd[k])) for k, g in zip(keys, grads)}
