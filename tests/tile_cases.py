"""numpy restatements of the two kernels of csrc/tiles.hip, written from the rule in the issue / DESIGN.md 4.7 and NOT from
shallow_ntc_amd.tiling: the geometry is spelled out again here, so a slip in the module's mirror does not cancel against itself.
Per axis: R = max(1, L // T); core r = [r T, (r + 1) T), the last to L; extent = core grown by O on interior sides; band between r
and r + 1 = [(r + 1) T - O, (r + 1) T + O), offset j: tile r + 1 weighs 2 j + 1, tile r weighs 4 O - (2 j + 1), denominator 4 O."""
import numpy as np


def extents(L, T, O):
    R = max(1, L // T)
    out = []
    for r in range(R):
        lo = r * T - (O if r > 0 else 0)
        hi = L if r == R - 1 else (r + 1) * T + O
        out.append((lo, hi))
    return out


def axis_weights(L, T, O):
    """int64 [R, L]: the weight of every tile at every position (0 outside its extent), and the denominators int64 [L]."""
    ext = extents(L, T, O)
    w = np.zeros((len(ext), L), np.int64)
    for r, (lo, hi) in enumerate(ext):
        w[r, lo:hi] = 1
    den = np.ones(L, np.int64)
    for r in range(len(ext) - 1):
        b = (r + 1) * T
        for j in range(2 * O):
            p = b - O + j
            w[r + 1, p], w[r, p], den[p] = 2 * j + 1, 4 * O - (2 * j + 1), 4 * O
    return w, den


def extract(x, T, O):
    """x [n, H, W, c] -> list over (image, row, col) of x[image, extent rows, extent cols] (slicing)."""
    n, H, W, _ = x.shape
    return [x[i, y0:y1, x0:x1] for i in range(n) for y0, y1 in extents(H, T, O) for x0, x1 in extents(W, T, O)]


def assemble(tiles, n, H, W, c, T, O, region=None):
    """``tiles``: uint8 [eh, ew, c] per (image, row, col), None = not decoded -> (uint8 [n, h, w, c] of the window, the number
    of window pixels that need a missing tile; those are 0).  int64 arithmetic: (sum_t w_t v_t + D // 2) // D."""
    ys, xs = extents(H, T, O), extents(W, T, O)
    wy, dy = axis_weights(H, T, O)
    wx, dx = axis_weights(W, T, O)
    acc = np.zeros((n, H, W, c), np.int64)
    lost = np.zeros((n, H, W), bool)
    k = 0
    for i in range(n):
        for r, (y0, y1) in enumerate(ys):
            for q, (x0, x1) in enumerate(xs):
                w2 = wy[r, y0:y1, None] * wx[q, None, x0:x1]
                if tiles[k] is None:
                    lost[i, y0:y1, x0:x1] |= w2 > 0
                else:
                    assert tiles[k].shape == (y1 - y0, x1 - x0, c)
                    acc[i, y0:y1, x0:x1] += w2[:, :, None] * tiles[k].astype(np.int64)
                k += 1
    D = (dy[:, None] * dx[None, :])[None, :, :, None]
    out = (acc + D // 2) // D
    out[lost] = 0
    y0, x0, h, w = (0, 0, H, W) if region is None else region
    return out[:, y0:y0 + h, x0:x0 + w].astype(np.uint8), int(lost[:, y0:y0 + h, x0:x0 + w].sum())
