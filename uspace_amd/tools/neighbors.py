"""Memorisation checks on the MI355X: the nearest training samples of every generated sample, and the two numbers the FD-DINOv2 /
PRDC literature prints beside its fidelity and diversity metrics -- the authenticity percentage and the data-copying test -- plus the
figure of generated samples next to their nearest training images.

All of it rests on one primitive, ``uspace_metric_topk`` (uspace_amd/csrc/metrics.hip): for every row of ``queries`` the k nearest
rows of ``bank`` WITH their indices, in the order (d2, index), selected on the fp64 Gram tiles (the nx x ny matrix is never
stored) and reported as the refined sum (x - y)^2 in fp64, so that an exact copy reports exactly 0.0.

  ``authenticity``     a generated sample is authentic when its distance to its nearest training sample i* is larger than i*'s
                       distance to its own nearest other training sample; the percentage of authentic samples.
  ``copying_zscore``   with L(a) the distance of a to its nearest training sample, Z_U of the Mann-Whitney statistic of L(generated)
                       against L(held-out real): negative when generated samples sit closer to the training set than held-out
                       real ones do.  With ``cells`` the per-cell form, averaged with the cells' share of the training set.

Both definitions are written from memory of the published ones (``AuthPct``; the data-copying test) and are NOT verified against
that code.  Inputs: ``FeatureBank``s, device tensors or arrays [n, F].  There is no CPU path: a CPU
tensor or a missing library raises ``UspaceHipError``."""
import math

import numpy as np
import torch

from uspace_amd import _hip
from uspace_amd.tools._inputs import ImagePathDataset, image_files, require_paths, rocm_device, uint8_batches
from uspace_amd.tools.feature_metrics import MAX_NEAREST_K, FeatureBank, _device_features, _features, bank_of_path

MIN_CELL = 10


def _set(a, name):
    return _features(torch.from_numpy(a) if isinstance(a, np.ndarray) else a, name)


def _on_device(t, a, name):
    """The checked set ``t`` of the argument ``a`` as contiguous fp32 on the device; an array has no device and goes to the ROCm one."""
    if isinstance(a, np.ndarray):
        t = t.to(rocm_device(None, "nearest neighbours"))
    return _device_features(t, name)


def _check_k(k):
    if int(k) != k or not 1 <= int(k) <= MAX_NEAREST_K:
        raise ValueError(f"k must be an integer in 1 .. {MAX_NEAREST_K}, got {k}")
    return int(k)


def merge_topk(d2_a, idx_a, d2_b, idx_b, k):
    """The k smallest by (d2, idx) of every row of two lists [n, ka], [n, kb] (tensors on one device): two stable sorts, by
    index and then by distance.  Empty slots (+inf, -1) sort behind every neighbour."""
    d2 = torch.cat([d2_a, d2_b], 1)
    idx = torch.cat([idx_a, idx_b], 1)
    by_idx = torch.sort(idx, dim=1, stable=True).indices
    d2, idx = d2.gather(1, by_idx), idx.gather(1, by_idx)
    by_d2 = torch.sort(d2, dim=1, stable=True).indices
    return d2.gather(1, by_d2)[:, :k].contiguous(), idx.gather(1, by_d2)[:, :k].contiguous()


@torch.no_grad()
def nearest_neighbors(queries, bank, k=1, exclude_self=False, shard_rows=None):
    """(d2 fp64 [nq, k], idx int32 [nq, k]) on the device: the k nearest rows of ``bank`` for every row of ``queries``, each row
    ascending in (d2, idx); fewer than k eligible rows leave (+inf, -1) at the end.  ``exclude_self``: ``queries`` IS ``bank``
    (row i of one is row i of the other) and row i is not its own neighbour.  ``shard_rows``: walk the bank that many rows at a
    time and merge the per-shard lists on the device; every shard reports refined distances, so the merge compares like with like
    and the result is the unsharded one wherever no two candidates lie within the selection's ceiling of each other."""
    q, b = _set(queries, "queries"), _set(bank, "bank")
    if q.shape[1] != b.shape[1]:
        raise ValueError(f"feature widths differ: {q.shape[1]} and {b.shape[1]}")
    if q.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError(f"both sets need at least one row, got {q.shape[0]} and {b.shape[0]}")
    k = _check_k(k)
    if exclude_self and q.shape[0] != b.shape[0]:
        raise ValueError(f"exclude_self needs the bank to be the query set, got {q.shape[0]} and {b.shape[0]} rows")
    if shard_rows is not None and (int(shard_rows) != shard_rows or int(shard_rows) < 1):
        raise ValueError(f"shard_rows must be a positive integer, got {shard_rows}")
    q, b = _on_device(q, queries, "queries"), _on_device(b, bank, "bank")
    self_base = 0 if exclude_self else -1
    step = b.shape[0] if shard_rows is None else int(shard_rows)
    d2 = idx = None
    for lo in range(0, b.shape[0], step):
        d, i = _hip.metric_topk(q, b[lo:lo + step], k, index_base=lo, self_base=self_base)
        d2, idx = (d, i) if d2 is None else merge_topk(d2, idx, d, i, k)
    return d2, idx


@torch.no_grad()
def authenticity(fake, train):
    """dict(authenticity_pct, authentic, d2, idx, train_d2): ``authentic`` bool [n_fake] on the device, true where the squared
    distance ``d2`` [n_fake] to the nearest training sample ``idx`` [n_fake] exceeds that sample's squared distance to its own
    nearest other training sample (``train_d2`` [n_train]); the percentage as a Python float."""
    f, t = _set(fake, "fake"), _set(train, "train")
    if f.shape[1] != t.shape[1]:
        raise ValueError(f"feature widths differ: {f.shape[1]} and {t.shape[1]}")
    if f.shape[0] < 1 or t.shape[0] < 2:
        raise ValueError(f"authenticity needs a generated sample and two training samples, got {f.shape[0]} and {t.shape[0]}")
    f, t = _on_device(f, fake, "fake"), _on_device(t, train, "train")
    d2, idx = nearest_neighbors(f, t, 1)
    train_d2, _ = nearest_neighbors(t, t, 1, exclude_self=True)
    d2, idx, train_d2 = d2[:, 0], idx[:, 0], train_d2[:, 0]
    authentic = d2 > train_d2[idx.long()]
    return dict(authenticity_pct=100.0 * int(authentic.sum()) / f.shape[0], authentic=authentic, d2=d2, idx=idx, train_d2=train_d2)


def mann_whitney_z(l_fake, l_test):
    """Z_U = (U - m n / 2) / sqrt(m n (m + n + 1) / 12) with U the number of pairs L(fake) > L(test), ties counting one half:
    fp64 on the host, from the mid-ranks of the pooled sample (U = R_fake - m (m + 1) / 2)."""
    a, b = np.asarray(l_fake, np.float64).ravel(), np.asarray(l_test, np.float64).ravel()
    m, n = len(a), len(b)
    if m < 1 or n < 1:
        raise ValueError(f"both samples need at least one value, got {m} and {n}")
    pooled = np.concatenate([a, b])
    values, inverse, counts = np.unique(pooled, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts).astype(np.float64)                     # rank of the last member of every tie group
    mid = ends - (counts - 1) / 2.0
    r_fake = mid[inverse[:m]].sum()
    u = r_fake - m * (m + 1) / 2.0
    return float((u - m * n / 2.0) / math.sqrt(m * n * (m + n + 1) / 12.0))


def _cell_labels(c, n, name):
    c = np.asarray(c.detach().cpu() if torch.is_tensor(c) else c)
    if c.shape != (n,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"{name} must hold one integer label per sample ({n}), got {c.dtype} {c.shape}")
    return c


@torch.no_grad()
def copying_zscore(fake, test, train, cells=None, min_cell=MIN_CELL):
    """Z_U of the data-copying test (a Python float).  ``cells=(cell_of_fake, cell_of_test, cell_of_train)``: integer labels of
    the caller's partition (e.g. its own k-means); Z_U of every cell that holds at least ``min_cell`` test and ``min_cell``
    generated samples, averaged with the cells' training-set counts as weights (normalised over the cells kept).  The distances are
    to the nearest sample of the whole training set.  Without ``cells`` there is one cell, whatever its size."""
    f, s, t = _set(fake, "fake"), _set(test, "test"), _set(train, "train")
    if not f.shape[1] == s.shape[1] == t.shape[1]:
        raise ValueError(f"feature widths differ: {f.shape[1]}, {s.shape[1]} and {t.shape[1]}")
    if min(f.shape[0], s.shape[0], t.shape[0]) < 1:
        raise ValueError("every set needs at least one row")
    if cells is not None:
        if len(cells) != 3:
            raise ValueError("cells must be (cell_of_fake, cell_of_test, cell_of_train)")
        if int(min_cell) != min_cell or int(min_cell) < 1:
            raise ValueError(f"min_cell must be a positive integer, got {min_cell}")
        cf, cs, ct = (_cell_labels(c, x.shape[0], n) for c, x, n in zip(cells, (f, s, t), ("cell_of_fake", "cell_of_test", "cell_of_train")))
        kept = [c for c in np.unique(ct) if (cf == c).sum() >= min_cell and (cs == c).sum() >= min_cell]
        if not kept:
            raise ValueError(f"no cell holds {min_cell} test and {min_cell} generated samples")
    f, s, t = _on_device(f, fake, "fake"), _on_device(s, test, "test"), _on_device(t, train, "train")
    l_fake = nearest_neighbors(f, t, 1)[0][:, 0].cpu().numpy()
    l_test = nearest_neighbors(s, t, 1)[0][:, 0].cpu().numpy()
    if cells is None:
        return mann_whitney_z(l_fake, l_test)
    z = np.array([mann_whitney_z(l_fake[cf == c], l_test[cs == c]) for c in kept])
    w = np.array([(ct == c).sum() for c in kept], np.float64)
    return float((z * w).sum() / w.sum())


def _bank_rows(bank_images, rows):
    """{row: image fp32 [3, H, W] in [0, 1] on the host} of the rows named, from a tensor [n, 3, H, W] or an image folder."""
    if torch.is_tensor(bank_images):
        return {j: bank_images[j].detach().float().cpu() for j in rows}
    files = image_files(bank_images)
    data = ImagePathDataset(files)
    for j in rows:
        if j >= len(files):
            raise ValueError(f"neighbour index {j} beyond the {len(files)} images of {bank_images}")
    return {j: data[j].float() / 255 for j in rows}


def neighbor_grid(query_images, bank_images, idx, path, padding=2, pad_value=1.0):
    """Write one PNG: row i is query image i followed by the bank images ``idx[i, :]`` (an empty slot, -1, stays ``pad_value``).
    ``query_images`` [n, 3, H, W] in [0, 1]; ``bank_images`` a tensor of such images or a folder (``fid_score``'s file order), of
    which only the rows named in ``idx`` are loaded.  Returns the grid [3, n (H + padding) + padding, (k + 1) (W + padding) + padding]."""
    from uspace_amd.tools.utils_vis import make_grid, save_grid_topil
    idx = np.asarray(idx.detach().cpu() if torch.is_tensor(idx) else idx)
    if idx.ndim == 1:
        idx = idx[:, None]
    if not torch.is_tensor(query_images) or query_images.dim() != 4 or idx.ndim != 2 or idx.shape[0] != query_images.shape[0]:
        raise ValueError("expected query images [n, 3, H, W] and indices [n, k]")
    if not torch.is_tensor(bank_images):
        require_paths([bank_images])
    elif idx.max(initial=-1) >= bank_images.shape[0]:
        raise ValueError(f"neighbour index {int(idx.max())} beyond the {bank_images.shape[0]} bank images")
    q = query_images.detach().float().cpu()
    rows = _bank_rows(bank_images, sorted({int(j) for j in idx.ravel() if j >= 0}))
    tiles = []
    for i in range(idx.shape[0]):
        tiles.append(q[i])
        for j in idx[i]:
            tile = rows[int(j)] if j >= 0 else torch.full_like(q[i], pad_value)
            if tile.shape != q[i].shape:
                raise ValueError(f"bank image {int(j)} is {tuple(tile.shape)}, the queries are {tuple(q[i].shape)}")
            tiles.append(tile)
    grid = make_grid(torch.stack(tiles), idx.shape[1] + 1, padding=padding, pad_value=pad_value)
    save_grid_topil(grid, path)
    return grid


def _bank(path, model, batch_size, dims, device, num_workers):
    from uspace_amd.tools.dino_metrics import DinoFeatures
    if isinstance(model, DinoFeatures) and not str(path).endswith(".npz"):
        bank = FeatureBank.of_width(model.dims, device)
        for batch in uint8_batches(image_files(path), batch_size):
            bank.update_features(model.features(batch.to(device).float() / 255, quantize=False))
        return bank
    return bank_of_path(path, model, batch_size, dims, device, num_workers)


def calculate_memorization_given_paths(paths, device=None, batch_size=50, dims=2048, num_workers=8, model=None, k=1, cells=None,
                                       min_cell=MIN_CELL, shard_rows=None):
    """The memorisation numbers of image folders or saved banks (.npz): ``paths`` = (generated, train) or (generated, train, test).
    ``model``: an ``InceptionV3`` (default: the pool features of width ``dims``) or a ``DinoFeatures`` extractor; nothing is
    downloaded.  Returns ``authenticity``'s dict plus ``neighbors`` = (d2, idx) [n_generated, k] and, with a test set, ``z_u``."""
    if len(paths) not in (2, 3):
        raise ValueError("paths must be (generated, train) or (generated, train, test)")
    k = _check_k(k)
    device = rocm_device(device, "memorisation checks")
    require_paths(paths)
    if model is None and not all(str(p).endswith(".npz") for p in paths):
        from uspace_amd.tools.inception import InceptionV3
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)
    banks = [_bank(p, model, batch_size, dims, device, num_workers) for p in paths]
    out = authenticity(banks[0], banks[1])
    out["neighbors"] = nearest_neighbors(banks[0], banks[1], k, shard_rows=shard_rows)
    if len(banks) == 3:
        out["z_u"] = copying_zscore(banks[0], banks[2], banks[1], cells=cells, min_cell=min_cell)
    return out


__all__ = ["nearest_neighbors", "merge_topk", "authenticity", "mann_whitney_z", "copying_zscore", "neighbor_grid",
           "calculate_memorization_given_paths", "MIN_CELL"]
