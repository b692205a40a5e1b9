"""The rule of the coded pixel residual layer (csrc/residual_rules.h, DESIGN.md 4.7 "residual layer") restated in numpy, and the
inputs the kernel tests share.  Integer arithmetic in int64 throughout; nothing here imports the product."""
import numpy as np

LEVELS, BINS = 8, 511


def pixels(x):
    """float32 image values -> uint8 as sntc_pixels_sse quantises them: (v + .5) 255 in float32, round half to even, saturate."""
    v = (np.asarray(x, np.float32) + np.float32(0.5)) * np.float32(255.0)
    return np.clip(np.rint(v), 0.0, 255.0).astype(np.int64)


def quantize(x8, b, delta):
    r = np.asarray(x8, np.int64) - np.asarray(b, np.int64)
    return np.sign(r) * ((np.abs(r) + delta) // (2 * delta + 1))


def q_max(delta):
    return (255 + delta) // (2 * delta + 1)


def reconstruct(b, q, delta):
    return np.clip(np.asarray(b, np.int64) + np.asarray(q, np.int64) * (2 * delta + 1), 0, 255)


def classes(base):
    """base uint8 [n, h, w, c] -> the class level c + k of every value, int64 like base."""
    b = np.asarray(base, np.int64)
    n, h, w, c = b.shape
    jl, jr = np.maximum(np.arange(w) - 1, 0), np.minimum(np.arange(w) + 1, w - 1)
    iu, id_ = np.maximum(np.arange(h) - 1, 0), np.minimum(np.arange(h) + 1, h - 1)
    a = np.abs(b[:, :, jr] - b[:, :, jl]) + np.abs(b[:, id_] - b[:, iu])
    level = np.where(a == 0, 0, np.minimum(LEVELS - 1, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1))
    assert all(((a >= (1 << (l - 1))) == (level >= l)).all() for l in range(1, LEVELS))       # log2 in floats: checked in integers
    return level * c + np.arange(c)


def histogram(q, cls, c):
    """-> int64 [n, 8 c, 511]: how many values of each class of each image took q = bin - 255."""
    n = q.shape[0]
    flat = (np.arange(n).reshape(n, 1, 1, 1) * (LEVELS * c) + cls) * BINS + q + BINS // 2
    return np.bincount(flat.reshape(-1), minlength=n * LEVELS * c * BINS).reshape(n, LEVELS * c, BINS)


def table_ids(cls, choice):
    """choice [n, 8 c] -> the table of every value."""
    n = cls.shape[0]
    return np.asarray(choice, np.int64)[np.arange(n).reshape(n, 1, 1, 1), cls]


def prices(tabs, cost_table):
    """Brute force: what every q in [-255, 255] costs under each of the 64 tables, the encoder's ESCAPE rule spelled out."""
    out = np.zeros((64, BINS), np.int64)
    for t in range(64):
        lo, f = tabs[t]
        cost = cost_table([tabs[t]]).astype(np.int64)
        for q in range(-255, 256):
            s = q - lo
            out[t, q + 255] = cost[len(f) - 1] if (s < 0 or s >= len(f) - 1) else cost[s]
    return out


def images(n, h, w, c, seed):
    """(x float32 [n, h, w, c], base uint8 like it) for the kernel tests: x from random uint8 -- with runs of floats whose
    (v + .5) 255 lands exactly on k + 0.5 and floats outside [-0.5, 0.5] --, base random with flat patches (a = 0), pure 0 and
    pure 255 against the opposite extreme of x, so r = +-255 occurs."""
    rng = np.random.default_rng(seed)
    x8 = rng.integers(0, 256, size=(n, h, w, c))
    x = (x8.astype(np.float64) / 255.0 - 0.5).astype(np.float32)
    flat = x.reshape(-1)
    k = rng.integers(0, 255, size=flat.size)
    tie = ((k + 0.5) / 255.0 - 0.5).astype(np.float32)                 # float32 candidates; those that are exact ties stay
    is_tie = (tie.astype(np.float32) + np.float32(0.5)) * np.float32(255.0) == (k + 0.5).astype(np.float32)
    pick = (rng.random(flat.size) < 0.25) & is_tie
    flat[pick] = tie[pick]
    out = rng.random(flat.size) < 0.05
    flat[out] = rng.choice(np.array([-3.0, -0.51, 0.51, 2.5, -0.5, 0.5], np.float32), size=int(out.sum()))
    base = rng.integers(0, 256, size=(n, h, w, c)).astype(np.uint8)
    base[:, : max(1, h // 3)] = (base[:, : max(1, h // 3)] // 64) * 64   # a smoother band: low levels
    if h * w >= 4:
        base[0, 0, :2] = 0
        x[0, 0, :2] = 0.5                                               # x8 = 255 over base 0: r = 255
        base[-1, -1, -2:] = 255
        x[-1, -1, -2:] = -0.5                                           # x8 = 0 under base 255: r = -255
        base[n // 2, h // 2, :] = 17                                    # a flat run inside a row
    return x, base
