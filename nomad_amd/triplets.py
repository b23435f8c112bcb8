"""(Anchor, Positive, Negative) rows from a table of NSIM values: the reference's ``src/utils/nsim_triplet_sampling.py:13-64``
restated over indices.  Host code, numpy only: it needs no GPU (``Nomad.mine_triplets`` feeds it the table ``Nomad.nsim`` made)."""
from __future__ import annotations

import numpy as np

COLUMNS = ("clip", "anchor", "positive", "negative", "anc_pos_dist", "anc_neg_dist")


def create_triplets(nsim, names=None, N: int = 1, hard_sampling: bool = True, margin: float = 0.05, rng=None):
    """nsim: a (B, C) table, ``nsim[b][c]`` the NSIM of clean clip b under condition c.  As the reference does, the clean clip
    itself joins each clip's pool at NSIM 1.0: member c < C is condition c, member C is the clean clip.  Per clip, N draws:

    * the anchor is drawn uniformly from the clip's pool;
    * the positive is the pool member nearest to the anchor in NSIM other than the anchor;
    * anchor and positive leave the pool and stay out for the clip's remaining draws (the reference's ``df_g`` shrinks across
      its N draws in the same way), whether or not the draw yields a row;
    * ``hard_sampling``: the negative is the nearest remaining member; otherwise it is drawn uniformly from the remaining members
      whose distance from the anchor is above the positive's distance plus ``margin``.

    Ties in "nearest" go to the lower member index.  The reference asserts positive distance < negative distance; a draw that
    cannot satisfy it - a tie between the two distances, an empty easy set, a pool of fewer than three members - is DROPPED and
    counted, where the reference would raise or sample from nothing.  A condition whose NSIM is NaN never enters the pool (the
    reference drops such rows afterwards).

    -> (table, dropped): ``table`` a dict of equally long arrays - ``clip``, ``anchor``, ``positive``, ``negative`` (int64; the
    last three are member indices of that clip) and ``anc_pos_dist``, ``anc_neg_dist`` (float64), rows in the order drawn;
    ``dropped`` the number of draws that gave no row, so ``len(table["clip"]) + dropped == B * N``.  names: an optional (B, C + 1)
    nested list of the members' names (the clean clip's last); the table then also has the lists ``Anchor``, ``Positive``,
    ``Negative``, the reference's columns.

    rng: a ``numpy.random.Generator``, a seed for one, or None (fresh entropy).  The same seed gives the same table.  The stream of
    pandas' ``DataFrame.sample`` is NOT reproduced: the rule is the reference's, the draws are not."""
    table = np.asarray(nsim, dtype=np.float64)
    if table.ndim != 2:
        raise ValueError(f"nsim must be a (B, C) table, got shape {table.shape}")
    B, C = table.shape
    N = int(N)
    margin = float(margin)
    if N < 1:
        raise ValueError(f"N must be at least 1, got {N}")
    if not (np.isfinite(margin) and margin >= 0.0):
        raise ValueError(f"margin must be finite and not negative, got {margin}")
    if names is not None and (len(names) != B or any(len(row) != C + 1 for row in names)):
        raise ValueError("names must hold C + 1 names per clip: the C conditions' and the clean clip's")
    gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    out = {k: [] for k in COLUMNS}
    dropped = 0
    for b in range(B):
        values = np.concatenate([table[b], [1.0]])
        pool = [c for c in range(C + 1) if not np.isnan(values[c])]
        for _ in range(N):
            if len(pool) < 3:
                dropped += 1
                continue
            anchor = pool[int(gen.integers(len(pool)))]
            rest = [c for c in pool if c != anchor]
            dist = np.abs(values[rest] - values[anchor])
            k = int(np.argmin(dist))                 # the first of equal distances: the lower member index
            positive, pos_dist = rest[k], float(dist[k])
            pool = [c for c in rest if c != positive]
            dist = np.abs(values[pool] - values[anchor])
            if hard_sampling:
                k = int(np.argmin(dist))
            else:
                far = np.flatnonzero(dist > pos_dist + margin)
                if far.size == 0:
                    dropped += 1
                    continue
                k = int(far[int(gen.integers(far.size))])
            negative, neg_dist = pool[k], float(dist[k])
            if not pos_dist < neg_dist:
                dropped += 1
                continue
            for key, v in zip(COLUMNS, (b, anchor, positive, negative, pos_dist, neg_dist)):
                out[key].append(v)
    result = {k: np.asarray(out[k], dtype=np.float64 if k.endswith("dist") else np.int64) for k in COLUMNS}
    if names is not None:
        for col, key in (("Anchor", "anchor"), ("Positive", "positive"), ("Negative", "negative")):
            result[col] = [names[b][m] for b, m in zip(result["clip"], result[key])]
    return result, dropped
