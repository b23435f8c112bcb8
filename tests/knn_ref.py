"""The contract of ``nomad_knn`` (include/nomad_hip.h) on a float64 distance matrix, in plain torch.  Imported by the tests like
``ref64`` and ``guard``; not a test module itself.

Neighbours of a row are the k columns smallest under the key (d, column) with a NaN distance ordered as +infinity - a stable
ascending sort of the row with NaN replaced by +inf -, the reported distance is the matrix's own value (NaN stays NaN), and the
score is the sequential float64 sum of the k distances, nearest first, from 0.0, divided by k."""
import torch


def knn_ref(dist: torch.Tensor, k: int):
    """dist (Na,Nb) float64 -> (knn_dist (Na,k) float64, knn_idx (Na,k) int32, score (Na,) float64), on dist's device."""
    assert dist.dim() == 2 and dist.dtype == torch.float64 and 1 <= k <= dist.shape[1]
    key = torch.where(torch.isnan(dist), torch.full_like(dist, float("inf")), dist)
    idx = torch.sort(key, dim=1, stable=True).indices[:, :k]
    knn_dist = torch.gather(dist, 1, idx)
    score = torch.zeros(dist.shape[0], dtype=torch.float64, device=dist.device)
    for r in range(k):            # one accumulator, r ascending: k dependent additions, not a tree
        score = score + knn_dist[:, r]
    # (a tensor divisor: torch divides a GPU tensor by a Python number as a product with its reciprocal, which is not the quotient)
    return knn_dist, idx.to(torch.int32), score / torch.full_like(score, float(k))


def same(x: torch.Tensor, y: torch.Tensor) -> bool:
    """Equal bit for bit where neither is NaN, NaN in the same places (the payload of a NaN is not part of the contract)."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if not x.is_floating_point():
        return bool(torch.equal(x, y))
    nx, ny = torch.isnan(x), torch.isnan(y)
    bits = torch.int64 if x.dtype == torch.float64 else torch.int32
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    return bool(torch.equal(nx, ny)) and bool(torch.equal(torch.where(nx, zero, x).view(bits), torch.where(ny, zero, y).view(bits)))
