"""A plain torch restatement of every stage of the bf16 forward (``forward_bf16_run``, nomad_hip.hip), each judged on the input
the GPU stage actually received, and the checker that holds a stage's output to float64.  Imported by
``test_bf16_stage_ref_host.py`` (CPU: the checker passes an emulated correct kernel and rejects nine mutations of it) and
``test_gpu_bf16_stages_f64.py`` (GPU: the 99 recorded stages of four geometries); not a test module itself.

Method.  Teacher forcing: a stage function takes the GPU's own input buffer (bf16 values) and the weights as the library holds
them, and is evaluated twice on the CPU - ``ref64.both``: everything in float64 (y64, the truth) and everything in fp32 (y32, what
plain fp32 arithmetic gets).  bf16 rounding therefore never accumulates across stages: what is left between the GPU's output and
y64 is the fp32-class arithmetic of ONE kernel and ONE rounding of its output.

The bound (derived, nothing measured on the GPU enters it).  A kernel whose output is stored as bf16 rounds an fp32 value v to
nearest, |v - y64| <= delta.  Half a bf16 ulp is at most 2^-8 |v| (8 significand bits: ulp = 2^-7 at the bottom of a binade), so

    |g - y64| <= 2^-8 |v| + delta <= 2^-8 |y64| + (1 + 2^-8) delta,
    delta = ref64.C * max|y32 - y64| + ref64.FLOOR * max|y64| + a_stage,

elementwise in |y64|, with the factor 1.02 on 2^-8 that test_conv0_on_the_matrix_cores gives it.  ref64.C = 8 and
ref64.FLOOR = 1e-7 are the project's constants for fp32 arithmetic (ref64.py); a_stage is the documented approximation of that
stage and nothing else:

    conv1..6, fc1, pos-conv   A_GELU = 5.6e-5: the one-transcendental bf16-output GELU against the erf GELU (gemm_f32.hip.h
                              gelu_bf16out, 5.5e-5; the value test_gpu_bf16.py uses)
    conv0                     A_GELU + 1.13 |scale| 2^-16 sum_k |x_k| |w_k|, elementwise: the matrix-core kernel multiplies the
                              hi / lo bf16 halves of waveform and weight and keeps x_hi w_hi + x_hi w_lo + x_lo w_hi
                              (frontend.hip.h).  Dropped: x_lo w_lo (|lo| <= 2^-9 |.|: 2^-18 |x w|) and what the second half
                              itself loses to its rounding (2^-9 |lo| <= 2^-18 |.| for x and for w) - 3 (1 + 2^-9) 2^-18 < 2^-16
                              of the tap magnitudes, times the GroupNorm scale, times the GELU's largest slope (1.129)
    attention                 2^-8 (P |V|) elementwise, in float64: the probabilities are rounded to bf16 before the PV product
                              (2^-9 relative each) and the row sums are taken from the rounded P (2^-9 relative on the quotient)
    everything else           0 (QKV, out_proj + residual, fc2 + residual, the projection, the LayerNorms: fp32 arithmetic on
                              bf16 inputs and one rounding)

Outputs stored as fp32 (scale, shift, embeddings) use ``ref64.check`` with ref64.C unchanged; the GroupNorm sums (float64 on the
GPU) are held to L0 2^-52 times the same sums of absolute values (L0 additions in double).  The pad frames of ``xpad`` must be
exactly zero.

Which term dominates: 2^-8 |y64| wherever |y64| > ~1e-2 (delta is 1e-5 .. 1e-4: fp32 sums over K <= 6144); below that the GELU
stages are bounded by A_GELU and the attention by its P |V| term, which is the larger one for every element of near-uniform
attention (|sum p v| << sum p |v|).

Weights.  ``Weights`` builds each fp32 weight the way ``nomad_create`` / ``nomad_enable_bf16`` do and rounds it to bf16 once; both
evaluations (float64 and fp32) take those bf16 values:
    q rows of the fused QKV weight   (q_w * 0.125f) * log2(e) in fp32, then bf16 (to_bf16_scaled_kernel); the q bias likewise,
                                     kept in fp32 (scale_head_kernel); k / v rows and biases unscaled
    pos-conv                         v * float(g[k] / ||v[:, :, k]||), the factor formed in double and the product in fp32
                                     (nomad_create), then bf16 (posconv_wfrag_kernel)
    conv1..6, projection, out_proj, fc1, fc2   bf16(w)
    conv0, every bias, LayerNorm / GroupNorm parameters, the head   fp32 as given.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

import ref64

A_GELU = 5.6e-5
HALF_ULP = 1.02 * 2.0 ** -8
LOG2E = 1.44269504088896341                       # attention_bf16_v3.hip.h kLog2e (rounded to fp32 where the library does)
LOG2E_F32 = torch.tensor(LOG2E, dtype=torch.float32)
CONV_K = (10, 3, 3, 3, 3, 2, 2)
P = "ssl_model."


def bf16v(x: torch.Tensor) -> torch.Tensor:
    """fp32 tensor holding the bf16 roundings (to nearest even) of x."""
    return x.float().bfloat16().float()


class Weights:
    """The weights of a state dict as ``nomad_enable_bf16`` leaves them on the device: bf16 values (held in fp32 tensors) for
    every matrix the bf16 forward multiplies on the matrix cores, fp32 for the rest.  Built on demand, cached."""

    def __init__(self, sd: Dict[str, torch.Tensor]):
        self.sd = sd
        self._c: Dict[str, object] = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def f32(self, key: str) -> torch.Tensor:
        return self.sd[key].detach().float().contiguous()

    def conv0(self):
        """(512, 10) fp32: the matrix-core kernel splits it into hi + lo itself."""
        return self._get("conv0", lambda: self.f32(P + "feature_extractor.conv_layers.0.0.weight").reshape(512, 10))

    def gn(self):
        return self.f32(P + "feature_extractor.conv_layers.0.2.weight"), self.f32(P + "feature_extractor.conv_layers.0.2.bias")

    def conv(self, i: int):
        """(512, k * 512), column t * 512 + ci = w[n][ci][t]: the K order of the implicit GEMM over time-major frames."""
        def make():
            w = self.f32(P + f"feature_extractor.conv_layers.{i}.0.weight")               # (512, 512, k)
            return bf16v(w.permute(0, 2, 1).reshape(512, CONV_K[i] * 512).contiguous())
        return self._get(f"conv{i}", make)

    def feature_ln(self):
        return self.f32(P + "layer_norm.weight"), self.f32(P + "layer_norm.bias")

    def proj(self):
        return self._get("proj", lambda: bf16v(self.f32(P + "post_extract_proj.weight"))), self.f32(P + "post_extract_proj.bias")

    def pos(self):
        """((768, 48, 128) weight-normed weight in bf16 values, (768,) fp32 bias)."""
        def make():
            v = self.f32(P + "encoder.pos_conv.0.weight_v")                               # (768, 48, 128)
            g = self.f32(P + "encoder.pos_conv.0.weight_g").flatten()                     # (128,)
            nrm = (v.double() ** 2).sum((0, 1))
            sc = (g.double() / nrm.sqrt()).float()
            return bf16v(v * sc)
        return self._get("pos", make), self.f32(P + "encoder.pos_conv.0.bias")

    def encoder_ln(self):
        return self.f32(P + "encoder.layer_norm.weight"), self.f32(P + "encoder.layer_norm.bias")

    def layer(self, l: int) -> Dict[str, torch.Tensor]:
        def make():
            q = P + f"encoder.layers.{l}."
            qw = (self.f32(q + "self_attn.q_proj.weight") * 0.125) * LOG2E_F32           # fp32 products, as the library forms them
            qb = (self.f32(q + "self_attn.q_proj.bias") * 0.125) * LOG2E_F32
            return {
                "qkv_w": bf16v(torch.cat([qw, self.f32(q + "self_attn.k_proj.weight"), self.f32(q + "self_attn.v_proj.weight")])),
                "qkv_b": torch.cat([qb, self.f32(q + "self_attn.k_proj.bias"), self.f32(q + "self_attn.v_proj.bias")]),
                "o_w": bf16v(self.f32(q + "self_attn.out_proj.weight")), "o_b": self.f32(q + "self_attn.out_proj.bias"),
                "ln1_w": self.f32(q + "self_attn_layer_norm.weight"), "ln1_b": self.f32(q + "self_attn_layer_norm.bias"),
                "fc1_w": bf16v(self.f32(q + "fc1.weight")), "fc1_b": self.f32(q + "fc1.bias"),
                "fc2_w": bf16v(self.f32(q + "fc2.weight")), "fc2_b": self.f32(q + "fc2.bias"),
                "ln2_w": self.f32(q + "final_layer_norm.weight"), "ln2_b": self.f32(q + "final_layer_norm.bias"),
            }
        return self._get(f"layer{l}", make)

    def head(self):
        return self.f32("embedding_layer.1.weight"), self.f32("embedding_layer.1.bias")


# ---- the stage functions: dtype-generic bodies (_name) and their (y64, y32) pairs ------------------------------------------
def gn_sums(wav: torch.Tensor):
    """Stage 0: per clip the 10 tap sums S_q = sum_t x[5 t + q] and the 55 products R_qk (q <= k, row-major) over the L0 conv0
    frames (frontend.hip.h wav_stats_kernel), in float64 -> (sums (B, 65), the same sums of absolute values)."""
    x = wav.double().unfold(1, 10, 5)                                                      # (B, L0, 10)
    iu = torch.triu_indices(10, 10)
    R =(x.transpose(1, 2) @ x)[:, iu[0], iu[1]]
    Ra = (x.abs().transpose(1, 2) @ x.abs())[:, iu[0], iu[1]]
    return torch.cat([x.sum(1), R], 1), torch.cat([x.abs().sum(1), Ra], 1)


def _gn_fold64(stats, w0, gamma, beta, L0):
    """gn_fold_kernel: mean and biased variance of conv0's output channel c from the tap sums, folded into
    scale = rstd * gamma, shift = beta - mean * rstd * gamma."""
    iu = torch.triu_indices(10, 10)
    w = w0.double()                                                                        # (512, 10)
    s1 = stats[:, :10] @ w.t()                                                             # (B, 512)
    ww = w[:, iu[0]] * w[:, iu[1]] * torch.where(iu[0] == iu[1], 1.0, 2.0).double()        # (512, 55)
    s2 = stats[:, 10:] @ ww.t()
    mean = s1 / L0
    var = (s2 / L0 - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    return rstd * gamma.double(), beta.double() - mean * rstd * gamma.double()


def gn_fold(stats: torch.Tensor, wav: torch.Tensor, w0, gamma, beta):
    """Stages 1, 2 -> ((scale64, shift64), (scale32, shift32)).  float64: gn_fold_kernel's formula on the GPU's own sums (its
    input).  fp32: the plain evaluation - conv0 in fp32, mean and biased variance of its output - since the sums do not exist in
    fp32 (the moment form cancels there)."""
    L0 = (wav.shape[1] - 10) // 5 + 1
    y64 = _gn_fold64(stats.double(), w0, gamma, beta, L0)
    vm = [torch.var_mean(x.unfold(0, 10, 5) @ w0.float().t(), 0, unbiased=False) for x in wav.float()]   # per clip: (L0, 512)
    var, mean = torch.stack([v for v, _ in vm]), torch.stack([m for _, m in vm])
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    return y64, (rstd * gamma.float(), beta.float() - mean * rstd * gamma.float())


def _conv0(xwin, scale, shift, w0):
    return F.gelu((xwin @ w0.t()) * scale + shift)


def conv0(xwin: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, w0: torch.Tensor):
    """Stage 3 on rows: xwin (R, 10) the samples 5 t .. 5 t + 9 of each output frame, scale / shift (R, 512) of the frame's clip
    (the GPU's own, stages 1 / 2) -> (y64, y32, a_stage) (R, 512)."""
    y64, y32 = ref64.both(_conv0, xwin, scale, shift, w0)
    a = A_GELU + 1.13 * scale.double().abs() * 2.0 ** -16 * (xwin.double().abs() @ w0.double().abs().t())
    return y64, y32, a


def conv_windows(x: torch.Tensor, k: int) -> torch.Tensor:
    """x (B, L, 512) time-major -> (B * Lout, k * 512): the frames 2 t .. 2 t + k - 1 of every output frame (stride 2)."""
    B = x.shape[0]
    return x.unfold(1, k, 2).permute(0, 1, 3, 2).reshape(B * ((x.shape[1] - k) // 2 + 1), k * 512)


def _conv(xwin, w):
    return F.gelu(xwin @ w.t())


def conv(xwin: torch.Tensor, w: torch.Tensor):
    """conv1..6 on rows: F.conv1d(x, w, stride=2) without bias over the time-major input, then the erf GELU, written as the
    implicit GEMM over each output frame's k input frames (test_bf16_stage_ref_host.py holds it equal to F.conv1d)."""
    return ref64.both(_conv, xwin, w)


def _layernorm(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def layernorm(x, g, b):
    return ref64.both(_layernorm, x, g, b)


def _linear(x, w, b, res=None, gelu=False):
    y = x @ w.t() + b
    if gelu:
        y = F.gelu(y)
    return y if res is None else y + res


def linear(x, w, b, res=None, gelu=False):
    """x W^T + b, then the erf GELU or the residual (QKV, projection; fc1; out_proj + x, fc2 + x2)."""
    return ref64.both(_linear, x, w, b, res, gelu=gelu)


def xpad_rows(xpad: torch.Tensor, b: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """xpad (16, B, T + 128, 48) group-major -> (R, 768): the projection's row of frame t of clip b, found at padded frame
    64 + t, channel 48 g + c in group g."""
    return xpad[:, b, 64 + t, :].permute(1, 0, 2).reshape(b.numel(), 768)


def xpad_windows(xpad: torch.Tensor, b: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """-> (R, 129, 768): the padded frames t .. t + 128 that output frames t and t + 1 of clip b read, channels 48 g + c."""
    fr = t[:, None] + torch.arange(129, device=t.device)[None, :]
    return xpad[:, b[:, None], fr, :].permute(1, 2, 0, 3).reshape(b.numel(), 129, 768)


def xpad_clips(xpad: torch.Tensor) -> torch.Tensor:
    """-> (B, T + 128, 768)."""
    return xpad.permute(1, 2, 0, 3).reshape(xpad.shape[1], xpad.shape[2], 768)


def _posconv(xp, w, bias):
    nb, tp, _ = xp.shape
    n_out = tp - 128                                                                       # tp - 127 outputs, the last one dropped
    out = []
    for g in range(16):
        a = xp[:, :, 48 * g:48 * g + 48].unfold(1, 128, 1)[:, :n_out]                     # (nb, n_out, 48 ci, 128 taps)
        wg = w[48 * g:48 * g + 48].reshape(48, 48 * 128)                                   # [n][ci * 128 + tap]
        out.append(a.reshape(nb * n_out, 48 * 128) @ wg.t())
    y = torch.cat(out, 1).reshape(nb, n_out, 768) + bias
    return xp[:, 64:64 + n_out] + F.gelu(y)


def posconv(xp: torch.Tensor, w: torch.Tensor, bias: torch.Tensor):
    """Conv1d(768, 768, k = 128, padding 64, groups 16) over frames that already carry their 64 zero pad frames per side, its
    last output dropped (SamePad), bias, the erf GELU, PLUS the layer's input (padded frame 64 + t): xp (clips, Tp, 768) ->
    (clips, Tp - 128, 768).  A whole clip is Tp = T + 128; a sampled frame is a window of Tp = 129."""
    return ref64.both(_posconv, xp, w, bias)


def _attention(q, k, v):
    """q (B, Tq, 768) carrying 64^-0.5 log2 e, k / v (B, T, 768) -> (ctx (B, Tq, 768), P |V|)."""
    B, Tq, T = q.shape[0], q.shape[1], k.shape[1]
    qh = (q / LOG2E).view(B, Tq, 12, 64).transpose(1, 2)
    kh, vh = (x.view(B, T, 12, 64).transpose(1, 2) for x in (k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2), -1)
    back = lambda o: o.transpose(1, 2).reshape(B, Tq, 768)
    return back(p @ vh), back(p @ vh.abs())


def attention(q, k, v):
    """-> (y64, y32, a_stage = 2^-8 P |V| in float64)."""
    (y64, pav), (y32, _) = ref64.both(_attention, q, k, v)
    return y64, y32, 2.0 ** -8 * pav


def _head(x, w, b):
    return F.normalize(F.relu(x.mean(1)) @ w.t() + b, dim=1)


def head(x, w, b):
    """x (B, T, 768) -> mean over T, ReLU, Linear(768, 256), L2 normalise."""
    return ref64.both(_head, x, w, b)


# ---- the checker -----------------------------------------------------------------------------------------------------------
class Report:
    """Per stage kind of one geometry: the worst err / bound, and (bf16 stages) the worst share of the fp32-class budget
    (1 + 2^-8) delta that an element needs beyond half an ulp of ITS OWN binade - err / bound alone sits at 1 / 1.02 for every
    large tensor, because some element always lies half an ulp from float64 at the bottom of a binade."""

    def __init__(self, case: str):
        self.case = case
        self.worst: Dict[str, float] = {}
        self.share: Dict[str, float] = {}

    def note(self, kind: str, ratio: float, share: Optional[float] = None):
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)
        if share is not None:
            self.share[kind] = max(self.share.get(kind, 0.0), share)

    def print(self):
        print(f"BF16 stages {self.case}: worst err / bound (share of delta)  " + "  ".join(
            f"{k} {v:.3f}" + (f" ({self.share[k]:.2f})" if k in self.share else "") for k, v in self.worst.items()))


def _delta(y64: torch.Tensor, y32: torch.Tensor, a_stage=0.0):
    top = y64.abs().max().item() if y64.numel() else 0.0
    e32 = (y32.double() - y64).abs().max().item() if y64.numel() else 0.0
    return ref64.C * e32 + ref64.FLOOR * top + a_stage


def bound_bf16(y64: torch.Tensor, y32: torch.Tensor, a_stage=0.0) -> torch.Tensor:
    return HALF_ULP * y64.abs() + (1.0 + 2.0 ** -8) * _delta(y64, y32, a_stage)


def check_bf16(kind: str, name: str, got: torch.Tensor, y64: torch.Tensor, y32: torch.Tensor, a_stage=0.0,
               report: Optional[Report] = None, rows: Optional[torch.Tensor] = None):
    """Assert |got - y64| <= bound_bf16 elementwise; the first offender is reported with its index (``rows``: the buffer row of
    each leading index, for sampled rows), the GPU's value and the reference's."""
    g = got.detach().cpu().double().reshape(y64.shape)
    assert torch.isfinite(g).all(), f"{name}: non-finite output"
    err = (g - y64).abs()
    bnd = bound_bf16(y64, y32, a_stage)
    ratio = (err / bnd).max().item() if err.numel() else 0.0
    if report is not None:
        big = torch.maximum(y64.abs(), g.abs())                 # the rounded value v lies in y64's binade or in the output's
        half = torch.where(big == 0, 0.0, torch.ldexp(torch.ones_like(y64), torch.frexp(big).exponent - 9))
        share = ((err - half) / ((1.0 + 2.0 ** -8) * _delta(y64, y32, a_stage))).max().item() if err.numel() else 0.0
        report.note(kind, ratio, max(share, 0.0))
    bad = err > bnd
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        where = list(i)
        if rows is not None:
            where[0] = int(rows.flatten()[i[0]])
        t = tuple(i)
        raise AssertionError(f"{name} [{kind}]: {int(bad.sum())} of {bad.numel()} elements outside the bound, first at {where}"
                             f" (sample {i}): got {g[t].item()!r} float64 {y64[t].item()!r} fp32 {float(y32[t])!r} "
                             f"err {err[t].item():.3e} bound {bnd[t].item():.3e}; worst err / bound {ratio:.2f}")


def check_f32(kind: str, name: str, got, y64, y32, report: Optional[Report] = None):
    """fp32 outputs: ref64.check, C unchanged."""
    res = ref64.check(name, got, y64, y32)
    if report is not None:
        report.note(kind, max(v[0] / v[2] for v in res.values()))


def check_sums(name: str, got: torch.Tensor, sums: torch.Tensor, sums_abs: torch.Tensor, L0: int, report: Optional[Report] = None):
    """The GroupNorm sums (float64 on the GPU): L0 additions in double."""
    g = got.detach().cpu().double().reshape(sums.shape)
    err, bnd = (g - sums).abs(), L0 * 2.0 ** -52 * sums_abs
    if report is not None:
        report.note("gn_sums", (err / bnd.clamp_min(1e-300)).max().item())
    bad = err > bnd
    if bad.any():
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} sums off, first at {list(i)}: got {g[i].item()!r} float64 {sums[i].item()!r}")


def check_zero(name: str, t: torch.Tensor):
    """Every element exactly zero (+0 or -0)."""
    nz = t != 0
    if bool(nz.any()):
        i = torch.nonzero(nz)[0].tolist()
        raise AssertionError(f"{name}: {int(nz.sum())} nonzero elements, first at {i}: {float(t[tuple(i)])!r}")
