"""Reference labeller for dmm_heat_components: plain numpy / Python, no scipy.  The oracle of tests/test_detect_gpu.py.

    labels, records, counts = heat_components(maps, threshold, connectivity=8, max_per_plane=1024)

maps: (B, NC, H, W) float32.  The semantics are those of include/dmmfods_hip.h, restated here:
  * foreground iff x >= threshold as fp32 values (a value on the threshold is in, NaN is out, -0.0 >= 0.0 holds);
  * components per (b, n) plane under 4- or 8-connectivity; rows do not wrap, planes never touch;
  * a component's label is its root, the smallest y * W + x among its pixels; background is -1;
  * records per plane in ascending root order; with more components than max_per_plane the smallest roots are kept, counts holds
    the true number, the slots behind min(count, max_per_plane) are zero;
  * score is the largest value in the order over bit patterns that puts -0.0 below +0.0, peak the first pixel in raster order that
    holds exactly that value (the same bits).
labels: int32 (B, NC, H, W); records: RECORD_DTYPE (B, NC, max_per_plane); counts: int32 (B, NC).
"""
import numpy as np

RECORD_DTYPE = np.dtype([("root", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area", "<i4"),
                         ("score", "<f4"), ("peak", "<i4")])
assert RECORD_DTYPE.itemsize == 32


def ordered_bits(values):
    """fp32 values -> uint32 keys whose integer order is the value order, -0.0 below +0.0."""
    b = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def label_plane(fg, connectivity):
    """fg: bool (H, W).  int32 (H, W): every foreground pixel's root, -1 elsewhere.  Union-find over one raster scan."""
    H, W = fg.shape
    parent = np.arange(H * W, dtype=np.int64)
    par = parent.tolist()
    f = fg.ravel().tolist()

    def find(x):
        r = x
        while par[r] != r:
            r = par[r]
        while par[x] != r:
            par[x], x = r, par[x]
        return r

    for y in range(H):
        for x in range(W):
            p = y * W + x
            if not f[p]:
                continue
            nbrs = []
            if x > 0:
                nbrs.append(p - 1)
            if y > 0:
                nbrs.append(p - W)
                if connectivity == 8:
                    if x > 0:
                        nbrs.append(p - W - 1)
                    if x < W - 1:
                        nbrs.append(p - W + 1)
            for q in nbrs:
                if f[q]:
                    a, b = find(p), find(q)
                    if a != b:   # the smaller index stays the root
                        if a < b:
                            par[b] = a
                        else:
                            par[a] = b
    out = np.full(H * W, -1, dtype=np.int32)
    for p in range(H * W):
        if f[p]:
            out[p] = find(p)
    return out.reshape(H, W)


def plane_records(values, labels, max_per_plane):
    """values fp32 (H, W), labels int32 (H, W) -> (records (max_per_plane,), true count)."""
    H, W = labels.shape
    rec = np.zeros(max_per_plane, dtype=RECORD_DTYPE)
    lab = labels.ravel()
    roots = np.unique(lab[lab >= 0])   # ascending
    keys = ordered_bits(values).ravel()
    vals = np.ascontiguousarray(values, dtype=np.float32).ravel()
    for slot, r in enumerate(roots[:max_per_plane]):
        idx = np.nonzero(lab == r)[0]   # ascending: raster order
        ys, xs = idx // W, idx % W
        k = keys[idx]
        peak = idx[np.nonzero(k == k.max())[0][0]]
        rec[slot] = (r, xs.min(), ys.min(), xs.max(), ys.max(), idx.size, vals[peak], peak)
    return rec, int(roots.size)


def heat_components(maps, threshold, connectivity=8, max_per_plane=1024):
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    maps = np.ascontiguousarray(maps, dtype=np.float32)
    B, NC, H, W = maps.shape
    labels = np.empty((B, NC, H, W), dtype=np.int32)
    records = np.zeros((B, NC, max_per_plane), dtype=RECORD_DTYPE)
    counts = np.zeros((B, NC), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        fg = maps >= np.float32(threshold)
    for b in range(B):
        for n in range(NC):
            labels[b, n] = label_plane(fg[b, n], connectivity)
            records[b, n], counts[b, n] = plane_records(maps[b, n], labels[b, n], max_per_plane)
    return labels, records, counts
