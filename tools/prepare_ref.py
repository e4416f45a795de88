"""Plain numpy restatements of the three rules of the device-side batch preparation (include/dmmfods_hip.h: dmm_prep_image,
dmm_prep_lidar, dmm_prep_heat_maps) - the oracle of tests/test_prepare_gpu.py.  Written from the rules as the header states
them; every result is exact, so the tests compare bit for bit.  tests/test_prepare_cpu.py holds these against torch's pooling layers
and against naive ordered loops."""
import numpy as np

F32 = np.float32


def image(src, pool):
    """src uint8 (H, W, C) -> float32 (C, Ho, Wo): float32(S) / float32(p * p), S the exact integer sum of the p x p block."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    H, W, C = src.shape
    p = int(pool)
    assert H % p == 0 and W % p == 0
    S = src.astype(np.int64).reshape(H // p, p, W // p, p, C).sum(axis=(1, 3))       # (Ho, Wo, C)
    out = S.astype(F32) / F32(p * p)                                                  # one IEEE fp32 division per element
    assert out.dtype == F32
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def lidar_owner(points, H, W, kernel_size=5):
    """int64 (H, W): the index of the highest-indexed valid point whose window covers the pixel, -1 where none does."""
    pts = np.asarray(points, dtype=F32).reshape(-1, 3)
    s = (int(kernel_size) - 1) // 2
    owner = np.full((H, W), -1, dtype=np.int64)
    for n, (x, y, d) in enumerate(pts):
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(d) and x >= 0 and y >= 0 and d >= 0):
            continue
        cx, cy = int(min(x, F32(2.0 ** 30))), int(min(y, F32(2.0 ** 30)))
        r0, r1 = max(cy - s, 0), min(cy + s + 1, H - 1)
        c0, c1 = max(cx - s, 0), min(cx + s + 1, W - 1)
        if r0 < r1 and c0 < c1:
            owner[r0:r1, c0:c1] = n      # (in list order: a later point overwrites)
    return owner


def lidar_code(values):
    """float32 plane of d (-1 where no point) -> the coded plane: two fp32 roundings per element."""
    v = np.asarray(values, dtype=F32)
    e = np.where(v == F32(-1), F32(76), np.minimum(v, F32(75))).astype(F32)
    near = (e * F32(-6.2)).astype(F32) + F32(255)
    far = (e * F32(-2)).astype(F32) + F32(150)
    return np.where(e <= F32(25), near, far).astype(F32)


def lidar(points, H, W, pool, kernel_size=5):
    """points (n, 3) float32 of (x, y, d) -> float32 (1, Ho, Wo)."""
    pts = np.asarray(points, dtype=F32).reshape(-1, 3)
    p = int(pool)
    assert H % p == 0 and W % p == 0 and (p == 1 or H >= 2 * p)
    owner = lidar_owner(pts, H, W, kernel_size)
    values = np.where(owner >= 0, pts[np.maximum(owner, 0), 2] if len(pts) else F32(-1), F32(-1)).astype(F32)
    code = lidar_code(values)
    if p == 1:
        return np.maximum(code, F32(0))[None]
    Ho, Wo = H // p, W // p
    out = np.empty((Ho, Wo), dtype=F32)
    for i in range(Ho):
        r = min(i, Ho - 2)
        win = code[r * p:r * p + 2 * p].reshape(2 * p, Wo, p)
        out[i] = np.maximum(win.max(axis=(0, 2)), F32(0))
    return out[None]


PLANE_OF_TYPE = {1: 0, 2: 1, 4: 2}


def pattern_at(type_, r, c, height, width):
    """float32: the value a box of this type and size gives the pixels at rows r (column vector) and columns c (row vector) from its corner."""
    pat = np.ones(np.broadcast(r, c).shape, dtype=F32)
    if type_ != 2:
        return pat
    hf, wf = height // 5, width // 4
    side = np.broadcast_to((c < wf) | (c >= 3 * wf), pat.shape)
    top, low = np.broadcast_to(r < hf, pat.shape), np.broadcast_to(r >= 3 * hf, pat.shape)
    pat[low & side] = F32(0.5)
    pat[low & ~side] = F32(0.75)
    pat[top & side] = F32(0.3)       # (top and low never both hold: hf > 0 gives hf <= 3 * hf, and with hf == 0 no r is below it)
    return pat


def box_pattern(type_, height, width):
    """float32 (height, width): the whole pattern of a box."""
    return pattern_at(type_, np.arange(height)[:, None], np.arange(width)[None, :], height, width)


def heat_maps_full(boxes, H, W):
    """boxes int (M, 5) of (type, x, y, width, height) -> float32 (3, H, W) at full resolution."""
    out = np.zeros((3, H, W), dtype=F32)
    for t, x, y, w, h in np.asarray(boxes, dtype=np.int64).reshape(-1, 5).tolist():
        if t not in PLANE_OF_TYPE or w <= 0 or h <= 0:
            continue
        y0, y1, x0, x1 = max(y, 0), min(y + h, H), max(x, 0), min(x + w, W)
        if y0 >= y1 or x0 >= x1:
            continue
        # the clipped part only (a box may be 2^31 wide), positioned relative to the unclipped corner; in list order: a later box of
        # the class overwrites
        out[PLANE_OF_TYPE[t], y0:y1, x0:x1] = pattern_at(t, (np.arange(y0, y1) - y)[:, None], (np.arange(x0, x1) - x)[None, :], h, w)
    return out


def heat_maps(boxes, H, W, pool):
    """boxes int (M, 5) -> float32 (3, Ho, Wo): the maximum of every p x p block of the full-resolution maps."""
    p = int(pool)
    assert H % p == 0 and W % p == 0
    full = heat_maps_full(boxes, H, W)
    return np.ascontiguousarray(full.reshape(3, H // p, p, W // p, p).max(axis=(2, 4)))


def batch(images, points, point_offsets, boxes, box_offsets, pool, kernel_size=5):
    """The (B, 3 + 1 + 3, Ho, Wo) float32 batch of B frames: images uint8 (B, H, W, 3), points / boxes concatenated with offsets."""
    images = np.asarray(images)
    B, H, W, C = images.shape
    p = int(pool)
    out = np.empty((B, C + 4, H // p, W // p), dtype=F32)
    pts, bxs = np.asarray(points, dtype=F32).reshape(-1, 3), np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    for b in range(B):
        out[b, :C] = image(images[b], p)
        out[b, C:C + 1] = lidar(pts[point_offsets[b]:point_offsets[b + 1]], H, W, p, kernel_size)
        out[b, C + 1:] = heat_maps(bxs[box_offsets[b]:box_offsets[b + 1]], H, W, p)
    return out
