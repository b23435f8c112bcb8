"""The patch-wise NSIM of include/nomad_hip.h (``nomad_nsim_patches``) restated in numpy; imported by the tests like ``nsim_ref``,
not a test module itself.  Activity, the kept table, the candidates (``nsim_ref.nsim_map`` on the cut-outs), the selection with its
order, and the results, in the header's order and in float64.  Nothing here is ViSQOL: the header's text is the definition, and
this file follows it line by line."""
import math

import numpy as np

import nsim_ref as N

BANDS = N.BANDS


def params(patch_s=0.4, search_s=1.2, vad_db=40.0, min_active=1.0):
    """Seconds and dB -> (patch, search, vad_ratio, min_active_frames) as ``Nomad.nsim_patches`` forms them: frames of 20 ms."""
    patch = int(round(patch_s * 50.0))
    search = int(round(search_s * 50.0))
    return patch, search, 10.0 ** (-vad_db / 10.0), max(1, int(math.ceil(min_active * patch)))


def energy(S):
    """E_t = sum_b S[t][b]^2, bands ascending from 0, each product rounded, then added."""
    S = np.asarray(S, dtype=np.float64)
    E = np.zeros(S.shape[0], dtype=np.float64)
    for b in range(BANDS):
        E = E + S[:, b] * S[:, b]
    return E


def activity(S, vad_ratio):
    """-> active [F] bool: E_t >= vad_ratio * max_t E_t (numpy's max carries a NaN; nothing is >= NaN)."""
    E = energy(S)
    with np.errstate(invalid="ignore"):
        return E >= np.float64(vad_ratio) * E.max()


def patch_count(F, patch):
    return F // patch


def window(p, patch, search, Fd):
    """[lo, hi] of patch p in a row of Fd frames; empty when lo > hi."""
    s = p * patch
    return max(s - search, 0), min(s + search, Fd - patch)


def kept_table(R, Fd, patch, search, vad_ratio, min_active_frames):
    """-> kept [P] bool for a row of Fd frames: enough active frames and a window that is not empty."""
    act = activity(R, vad_ratio)
    P = patch_count(R.shape[0], patch)
    out = np.zeros(P, dtype=bool)
    for p in range(P):
        lo, hi = window(p, patch, search, Fd)
        out[p] = int(act[p * patch:(p + 1) * patch].sum()) >= min_active_frames and lo <= hi
    return out


def candidates(R, D, patch, search, kept, intensity_range=1.0, dtype=np.float64):
    """-> (cand [P][2 search + 1], bands [P][2 search + 1][21]): q_p[u] at column u - (s - search), NaN where there is no candidate."""
    P = patch_count(R.shape[0], patch)
    cand = np.full((P, 2 * search + 1), np.nan, dtype=dtype)
    bands = np.full((P, 2 * search + 1, BANDS), np.nan, dtype=dtype)
    for p in range(P):
        if not kept[p]:
            continue
        s = p * patch
        lo, hi = window(p, patch, search, D.shape[0])
        for u in range(lo, hi + 1):
            q, bq, _ = N.nsim_map(R[s:s + patch], D[u:u + patch], intensity_range, dtype=dtype)
            cand[p, u - (s - search)] = q
            bands[p, u - (s - search)] = bq
    return cand, bands


def better(T, search, x, y):
    """Column x ahead of column y (None: nothing yet): larger T, then nearer to the patch's own start, then the earlier place."""
    if y is None:
        return True
    if T[x] != T[y]:
        return bool(T[x] > T[y])
    dx, dy = abs(x - search), abs(y - search)
    return dx < dy if dx != dy else x < y


def select(cand, kept, patch, search, Fd):
    """The chain over the kept patches -> (T_best, K, columns [P], -1 where not kept): T_0 = q_0; T_k[u] = T_{k-1}[a_k(u)] + q_k[u],
    a_k(u) the best u' in [lo_{k-1}, min(u, hi_{k-1})]; ends at the best place of the last window, traced back through a."""
    P = len(kept)
    cols = np.full(P, -1, dtype=np.int64)
    order = [p for p in range(P) if kept[p]]
    if not order:
        return float("nan"), 0, cols
    T, back = {}, {}
    for k, p in enumerate(order):
        s = p * patch
        lo, hi = window(p, patch, search, Fd)
        T[p] = np.full(2 * search + 1, np.nan)
        back[p] = np.full(2 * search + 1, -1, dtype=np.int64)
        if k == 0:
            for u in range(lo, hi + 1):
                T[p][u - (s - search)] = cand[p, u - (s - search)]
            continue
        pp = order[k - 1]
        sp = pp * patch
        plo, phi = window(pp, patch, search, Fd)
        for u in range(lo, hi + 1):
            best = None
            for v in range(plo, min(u, phi) + 1):
                if better(T[pp], search, v - (sp - search), best):
                    best = v - (sp - search)
            c = u - (s - search)
            back[p][c] = best
            T[p][c] = T[pp][best] + cand[p, c]
    last = order[-1]
    lo, hi = window(last, patch, search, Fd)
    best = None
    for u in range(lo, hi + 1):
        if better(T[last], search, u - (last * patch - search), best):
            best = u - (last * patch - search)
    total = T[last][best]
    for k in range(len(order) - 1, -1, -1):
        cols[order[k]] = best
        best = back[order[k]][best]
    return total, len(order), cols


def results(cand, cand_bands, kept, patch, search, Fd, clean_bad=False):
    """-> dict(nsim, bands [21], offsets [P] (-1 where not kept), patch_nsim [P] (NaN where not kept), kept K) from a row's
    candidate table: the header's "Results per row" and "Non-finite values"."""
    P = len(kept)
    void = dict(nsim=float("nan"), bands=np.full(BANDS, np.nan), offsets=np.full(P, -1, dtype=np.int64), patch_nsim=np.full(P, np.nan), kept=0)
    if clean_bad:
        return void
    for p in range(P):
        if kept[p]:
            lo, hi = window(p, patch, search, Fd)
            s = p * patch
            if np.isnan(cand[p, lo - (s - search):hi - (s - search) + 1]).any():
                return void
    total, K, cols = select(cand, kept, patch, search, Fd)
    if K == 0:
        return void
    bands = np.zeros(BANDS, dtype=np.float64)
    offsets = np.full(P, -1, dtype=np.int64)
    pn = np.full(P, np.nan)
    for p in range(P):                                                      # ascending kept patches
        if cols[p] >= 0:
            bands = bands + cand_bands[p, cols[p]]
            offsets[p] = p * patch - search + cols[p]
            pn[p] = cand[p, cols[p]]
    return dict(nsim=total / np.float64(K), bands=bands / np.float64(K), offsets=offsets, patch_nsim=pn, kept=K)


def nsim_patches_of_spectrograms(R, D, patch, search, vad_ratio, min_active_frames, intensity_range=1.0):
    """The whole measure for one pair of float64 spectrograms -> the dict of ``results`` plus ``cand`` and ``kept_table``."""
    R, D = np.asarray(R, dtype=np.float64), np.asarray(D, dtype=np.float64)
    if D.shape[0] < 1:
        raise ValueError("a degraded row needs a frame")
    kept = kept_table(R, D.shape[0], patch, search, vad_ratio, min_active_frames)
    cand, cand_bands = candidates(R, D, patch, search, kept, intensity_range)
    res = results(cand, cand_bands, kept, patch, search, D.shape[0], clean_bad=bool(np.isnan(R).any()))
    res["cand"], res["kept_table"], res["cand_bands"] = cand, kept, cand_bands
    return res


def nsim_patches(clean, degraded, fs=16000, patch_s=0.4, search_s=1.2, vad_db=40.0, min_active=1.0, intensity_range=1.0,
                 dtype=np.float64):
    """From the waveforms: spectrograms in ``dtype`` (float64: what the device computes), then the measure."""
    patch, search, ratio, need = params(patch_s, search_s, vad_db, min_active)
    R = N.spectrogram(clean, fs, dtype=dtype).astype(np.float64)
    D = N.spectrogram(degraded, fs, dtype=dtype).astype(np.float64)
    return nsim_patches_of_spectrograms(R, D, patch, search, ratio, need, intensity_range)


def jump_copy(x, first=2, second=3, H=320):
    """The copy that is late by ``first`` frames in its first half and by ``first + second`` in its second:
    zeros(first H) + x[:half] + zeros(second H) + x[half:], half = (n // 2) // H * H."""
    x = np.asarray(x, dtype=np.float32)
    half = (x.shape[0] // 2) // H * H
    return np.concatenate([np.zeros(first * H, np.float32), x[:half], np.zeros(second * H, np.float32), x[half:]])
