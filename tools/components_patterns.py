"""The input patterns of the connected-components tests, shared by tests/test_detect_cpu.py (the reference labeller against
scipy) and tests/test_detect_gpu.py (the kernels against the reference labeller).  Every pattern is a dict:
    name, maps (B, NC, H, W) float32, threshold, and optionally count8 / count4: the number of components of plane (0, 0) that the
    construction itself guarantees under 8- / 4-connectivity.
TH, TW are the tile extents of the kernels (DMM_CC_TILE_H, DMM_CC_TILE_W): the shapes are built from them so that chains cross tile
borders in both directions, corners meet diagonally across four tiles and the last tile row / column is ragged."""
import numpy as np


def _maps(fg, hi=1.0, lo=0.0):
    fg = np.asarray(fg, dtype=bool)
    while fg.ndim < 4:
        fg = fg[None]
    return np.where(fg, np.float32(hi), np.float32(lo)).astype(np.float32)


def spiral_path(H, W):
    """The pixels, in walking order, of a one-pixel-wide clockwise spiral from (0, 0) inwards whose arms stay one background pixel apart."""
    g = np.zeros((H, W), dtype=bool)
    y, x, d = 0, 0, 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    g[0, 0] = True
    path = [(0, 0)]

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and not g[yy, xx]

    def can(d):
        dy, dx = step[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        return free(y1, x1) and (not (0 <= y2 < H and 0 <= x2 < W) or not g[y2, x2])
    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                break
        y, x = y + step[d][0], x + step[d][1]
        g[y, x] = True
        path.append((y, x))
    return path


def _from_path(H, W, path):
    g = np.zeros((H, W), dtype=bool)
    for y, x in path:
        g[y, x] = True
    return g


def pedestrian_fill(h, w):
    """The reference's pedestrian box (create_ground_truth_maps): ones, the two upper corners (h // 5 rows, w // 4 columns) at 0.3,
    in the rows from 3 * (h // 5) on the outer quarters at 0.5 and the middle at 0.75.  Vehicles and cyclists are plain ones."""
    box = np.ones((h, w), dtype=np.float32)
    hf, wf = h // 5, w // 4
    box[:hf, :wf] = 0.3
    box[:hf, wf * 3:] = 0.3
    box[hf * 3:, :wf] = 0.5
    box[hf * 3:, wf * 3:] = 0.5
    box[hf * 3:, wf:wf * 3] = 0.75
    return box


def rectangles(H, W, seed, per_class=6):
    """Three class planes (vehicle, pedestrian, cyclist fills) of random rectangles that keep at least one background pixel between
    them.  Returns (maps (1, 3, H, W), boxes: per class a list of (y, x, h, w))."""
    rng = np.random.default_rng(seed)
    maps = np.zeros((1, 3, H, W), dtype=np.float32)
    boxes = [[], [], []]
    for c in range(3):
        used = np.zeros((H, W), dtype=bool)
        tries = 0
        while len(boxes[c]) < per_class and tries < 1000:
            tries += 1
            h, w = int(rng.integers(5, max(6, H // 3))), int(rng.integers(4, max(5, W // 3)))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            if used[max(0, y - 1):y + h + 1, max(0, x - 1):x + w + 1].any():
                continue
            used[y:y + h, x:x + w] = True
            maps[0, c, y:y + h, x:x + w] = pedestrian_fill(h, w) if c == 1 else 1.0
            boxes[c].append((y, x, h, w))
    return maps, boxes


def value_plane():
    """Threshold 0.0: values on the threshold, -0.0, NaN inside and beside a blob, infinities, subnormals, a maximum that occurs twice."""
    nan, inf = np.float32("nan"), np.float32("inf")
    sub = np.float32(1e-45)   # the smallest subnormal
    m = np.full((24, 40), -1.0, dtype=np.float32)
    m[1:4, 1:6] = 0.0                      # a blob of values exactly on the threshold ...
    m[2, 3] = -0.0                         # ... one of them -0.0: still foreground
    m[6:10, 2:9] = 0.5                     # a blob with a NaN hole and NaN beside it
    m[7, 4] = nan
    m[8, 9] = nan
    m[6, 12:15] = (0.25, 2.0, 2.0)         # the maximum twice: peak is the first
    m[7, 12:15] = (2.0, 1.0, 0.5)
    m[12, 1:5] = (sub, -sub, sub, 0.0)     # -subnormal is background: two components
    m[14, 1:4] = (1.0, inf, 3.0)           # +inf is the score
    m[16, 1:4] = (1.0, -inf, 1.0)          # -inf is background
    m[18, 1:4] = (-0.0, -0.0, -0.0)        # a component of -0.0 only: its score is -0.0
    m[20, 1:4] = (-0.0, 0.0, -0.0)         # +0.0 orders above -0.0
    m[22, 30:38] = nan                     # a row of NaN: nothing
    return m[None, None]


def patterns(TH, TW):
    out = []

    def add(name, maps, threshold=0.5, **kw):
        out.append(dict(name=name, maps=np.ascontiguousarray(maps, dtype=np.float32), threshold=threshold, **kw))

    # long chains
    H, W = 3 * TH + 5, 2 * TW + 3
    path = spiral_path(H, W)
    add("spiral", _maps(_from_path(H, W, path)), count8=1, count4=1)
    cut = path[:len(path) // 2] + path[len(path) // 2 + 1:]
    add("spiral_cut", _maps(_from_path(H, W, cut)), count8=2, count4=2)
    # late equivalences
    H, W = 2 * TH + 3, 2 * TW + 3
    comb = np.zeros((H, W), dtype=bool)
    comb[:, ::2] = True
    comb[-1, :] = True
    add("comb", _maps(comb), count8=1, count4=1)
    add("comb_upside_down", _maps(comb[::-1]), count8=1, count4=1)
    # tile corners
    c = np.zeros((2, 2 * TH, 2 * TW), dtype=bool)
    c[0, TH - 1, TW - 1] = c[0, TH, TW] = True
    c[1, TH - 1, TW] = c[1, TH, TW - 1] = True
    add("corners", _maps(c[None]), count8=1, count4=2)
    n = 3 * min(TH, TW)
    st = np.zeros((3 * TH, 3 * TW), dtype=bool)
    st[np.arange(n), np.arange(n)] = True
    add("staircase", _maps(st), count8=1, count4=n)
    # checkerboard
    H, W = 2 * TH + 1, 2 * TW + 1
    yy, xx = np.mgrid[:H, :W]
    add("checkerboard", _maps((yy + xx) % 2 == 0), count8=1, count4=(H * W + 1) // 2)
    # degenerate planes
    add("all_foreground", _maps(np.ones((2 * TH + 3, TW + 5), dtype=bool)), count8=1, count4=1)
    add("no_foreground", _maps(np.zeros((TH + 3, TW + 5), dtype=bool)), count8=0, count4=0)
    add("one_pixel", _maps(np.ones((1, 1), dtype=bool)), count8=1, count4=1)
    row = np.ones((1, 2 * TW + 3), dtype=bool)
    row[0, TW + 1] = False
    add("one_row", _maps(row), count8=2, count4=2)
    col = np.ones((2 * TH + 3, 1), dtype=bool)
    col[TH - 1, 0] = False
    add("one_column", _maps(col), count8=2, count4=2)
    rng = np.random.default_rng(11)
    add("smaller_than_a_tile", rng.uniform(0, 1, (1, 2, 5, 7)).astype(np.float32))
    add("width_not_a_multiple_of_four", rng.uniform(0, 1, (1, 1, TH + 2, TW + 6)).astype(np.float32), threshold=0.45)
    add("width_a_multiple_of_four", rng.uniform(0, 1, (2, 1, TH + 2, TW + 8)).astype(np.float32), threshold=0.45)
    # plane and row isolation: B = 2, NC = 3
    H, W = TH + 3, TW + 5
    iso = np.zeros((2, 3, H, W), dtype=bool)
    iso[:, :, 0, :] = iso[:, :, H - 1, :] = True
    iso[:, :, 5, W - 1] = iso[:, :, 6, 0] = True
    add("isolation", _maps(iso), count8=4, count4=4)
    # values
    add("values", value_plane(), threshold=0.0)
    # tangled input
    H, W = 3 * TH + 1, 3 * TW + 2
    for pct, thr in ((50, 0.5), (60, 0.4)):
        for seed in range(3):
            add(f"noise{pct}_seed{seed}", np.random.default_rng(100 * pct + seed).uniform(0, 1, (1, 1, H, W)).astype(np.float32), threshold=thr)
    # rectangles with the reference's fills, cut at 0.7
    maps, boxes = rectangles(3 * TH + 7, 4 * TW + 4, seed=5)
    add("rectangles", maps, threshold=0.7, boxes=boxes)
    return out
