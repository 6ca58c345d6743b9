"""Frames in overlapping tiles, restated (csrc/frame_stitch.hip): the tile grid and the blend weights in numpy,
written from the definition and not from the library's code, and the stitch as a loop in torch that takes a table as it is."""
import numpy as np
import torch


def origins(n, tile, overlap):
    """k * step for every k * step < n - tile, then n - tile; [0] when tile >= n."""
    if tile >= n:
        return [0]
    step, out, k = tile - overlap, [], 0
    while k * step < n - tile:
        out.append(k * step)
        k += 1
    return out + [n - tile]


def dense_weights(n, tile, overlap, scale):
    """float64 [scale * n, tiles]: w_k(r) = u_k(r) / sum_j u_j(r), u_k(r) = min(dl, dr) inside tile k and 0 outside."""
    org = origins(n, tile, overlap)
    L, N = scale * min(tile, n), scale * n
    u = np.zeros((N, len(org)), dtype=np.float64)
    r = np.arange(N, dtype=np.float64)
    for k, o in enumerate(org):
        O = scale * o
        dl = np.full(N, float(L)) if k == 0 else r - O + 0.5
        dr = np.full(N, float(L)) if k == len(org) - 1 else O + L - r - 0.5
        inside = (r >= O) & (r < O + L)
        u[:, k] = np.where(inside, np.minimum(dl, dr), 0.0)
    return u / u.sum(1, keepdims=True)


def table(n, tile, overlap, scale):
    """(origins in SR pixels int32 [tiles], first int32 [N], weights fp32 [N, K]) from dense_weights."""
    w = dense_weights(n, tile, overlap, scale)
    covers = w > 0
    K = int(covers.sum(1).max())
    first = covers.argmax(1).astype(np.int32)
    out = np.zeros((w.shape[0], K), dtype=np.float32)
    for r in range(w.shape[0]):
        m = int(covers[r].sum())
        assert covers[r, first[r]:first[r] + m].all()                  # the covering tiles are consecutive
        out[r, :m] = w[r, first[r]:first[r] + m].astype(np.float32)
    return np.asarray([scale * o for o in origins(n, tile, overlap)], dtype=np.int32), first, out


def dense_of(table_, tiles):
    """float32 [N, tiles] from a (origins, first, weights) table: the weight of every tile at every position."""
    _, first, weights = (np.asarray(t) for t in table_)
    out = np.zeros((first.shape[0], tiles), dtype=np.float32)
    for r in range(first.shape[0]):
        for a in range(weights.shape[1]):
            if weights[r, a] != 0:
                out[r, first[r] + a] = weights[r, a]
    return out


def stitch_torch(tiles, ny, nx, rows, cols):
    """tiles fp32 [ny * nx, planes, Ht, Wt] -> [planes, H, W] with the tables as they are (torch tensors on any device):
    dst[p, r, c] = sum_a sum_b (wy[r, a] * wx[c, b]) * tile(first_y[r] + a, first_x[c] + b)[p, r - O_y, c - O_x], a outer, b
    inner, every product and sum a torch fp32 op of its own, the accumulator starting as the first term; an entry whose row or
    column weight is 0 is not added (torch.where: its value, NaN or not, plays no part).  Columns go in chunks of 4, as the
    kernel's 16-byte accesses do: origins are multiples of 4, so the four columns of a chunk share their covering tiles --
    first_x is read at the chunk's first column, and a column index is clamped into the tile chunk-wise (rows one by one).
    For a table of the library's neither makes a difference."""
    dev = tiles.device
    oy, fy, wy = (t.to(dev) for t in rows)
    ox, fx, wx = (t.to(dev) for t in cols)
    H, W = fy.shape[0], fx.shape[0]
    Ht, Wt = tiles.shape[-2:]
    r, c = torch.arange(H, device=dev), torch.arange(W, device=dev)
    acc = torch.zeros((tiles.shape[1], H, W), dtype=torch.float32, device=dev)
    have = torch.zeros((H, W), dtype=torch.bool, device=dev)
    for a in range(wy.shape[1]):
        ty = (fy.long().clamp(0, ny - 1) + a).clamp(max=ny - 1)
        lr = (r - oy.long()[ty]).clamp(0, Ht - 1)
        for b in range(wx.shape[1]):
            tx = (fx.long()[c // 4 * 4].clamp(0, nx - 1) + b).clamp(max=nx - 1)
            lc = (c // 4 * 4 - ox.long()[tx]).clamp(0, Wt - 4) // 4 * 4 + c % 4
            val = tiles[(ty[:, None] * nx + tx[None, :]), :, lr[:, None], lc[None, :]].permute(2, 0, 1)   # [planes, H, W]
            w = wy[:, a][:, None] * wx[:, b][None, :]
            term = w * val
            use = (wy[:, a] != 0)[:, None] & (wx[:, b] != 0)[None, :]
            acc = torch.where(use, torch.where(have, acc + term, term), acc)
            have = have | use
    return acc


def data(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
