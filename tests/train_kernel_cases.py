"""Case tables, input builders and float64 references of the training step's small kernels (csrc/train.hip, csrc/wgrad.hip,
the backward half of csrc/sga.hip).  Shared by tests/test_hip_train_kernels.py (the kernels on the device) and
tests/test_train_kernels_host.py (the inputs' preconditions and the references themselves, on the CPU).

Every reference is float64 NumPy, or float64 autograd of the functions of oracle/train_ref.py.  Every builder is cached:
a reference is computed once per process and never written to.

The per-element bar of a kernel that is a fixed sequence of IEEE float32 operations is  |got - ref| <= r * 2^-24 * S:
S = float64 sum of the absolute values of the terms that enter the element, r = float32 roundings on its longest
path (a K-term accumulation in any order: K + 1).  The library is built with -ffp-contract=off and correctly rounded
division and square root, so every operation rounds once."""
import functools
import math

import numpy as np
import torch

from oracle import train_ref

U = 2.0 ** -24                     # unit roundoff of float32

# csrc/train.hip tr_grid(): `b > 2048 ? 2048 : b` blocks of 256 threads -- one trip of a grid-stride loop covers this many elements
TR_CAP = 2048 * 256
# csrc/sga.hip grid_for(): `b > 1024 ? 1024 : b` blocks of 256 threads (tail_bwd_kernel, adam_kernel); sntc_sumsq launches
# std::min(tr_grid(total), 1024) blocks as well
SGA_CAP = 1024 * 256

EW_SIZES = (1, 255, 257, 2 * TR_CAP + 259)      # 2 cap + 259: three trips for some threads, two for others, total % 4 == 3
EW_ZEROS = 64                                   # exact zeros of each sign wherever the size has room for them (>= 255)

GDN_BETA_MIN = 1e-6
GDN_PEDESTAL = np.float32(train_ref.GDN_OFFSET ** 2)
GDN_BOUND = np.float32(math.sqrt(GDN_BETA_MIN + train_ref.GDN_OFFSET ** 2))      # what train.py hands sntc_gdn_reparam_*


def f64(a):
    return np.asarray(a, dtype=np.float64)


def worst_ratio(got, ref, r, S):
    """max over elements of |got - ref| / (r 2^-24 S); elements with S == 0 must be exact.  <= 1 passes the bar."""
    err = np.abs(f64(got) - f64(ref))
    bar = r * U * f64(S)
    if not np.all(err[bar == 0] == 0):
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar > 0, err / bar, 0.0)
    return float(q.max()) if q.size else 0.0


def rel(a, b):
    """The statistic of tests/test_hip_train.py: max|got - ref| / max|ref|."""
    return float(np.abs(f64(a) - f64(b)).max() / max(np.abs(f64(b)).max(), 1e-30))


def _with_zeros(rng, a, count):
    """``count`` exact +0.0 and ``count`` exact -0.0 at random places of the flat float32 array ``a``."""
    idx = rng.permutation(a.size)[:2 * count]
    a.reshape(-1)[idx[:count]] = 0.0
    a.reshape(-1)[idx[count:]] = -0.0
    return a


def count_zeros(a):
    """(number of +0.0, number of -0.0)"""
    z = a == 0
    neg = np.signbit(a)
    return int((z & ~neg).sum()), int((z & neg).sum())


# ---- 1. element-wise kernels of train.hip --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def elementwise_inputs(total):
    rng = np.random.default_rng(4000 + total % 1009)
    nz = EW_ZEROS if total >= 255 else 0
    n = lambda: rng.standard_normal(total).astype(np.float32)
    d = dict(g=n(), t=n(), b=n())
    d["x"] = _with_zeros(rng, n(), nz)                       # sign(x), |x|
    d["y"] = _with_zeros(rng, n(), nz)                       # a layer output: relu / leaky_relu masks
    d["s"] = (1.0 / (1.0 + np.exp(-f64(n())))).astype(np.float32)          # a sigmoid output, in (0, 1)
    d["norm"] = (1e-3 + 2.0 * rng.random(total)).astype(np.float32)        # beta >= 1e-3 plus a non-negative sum
    d["noise"] = rng.uniform(-0.5, 0.5, total).astype(np.float32)
    # GDN reparameterisation: raw below / at / above the bound, g_eff of both signs, all four classes everywhere
    cls = rng.permutation(total) % 4                         # a quarter of the elements in each class
    raw = np.where(cls < 2, rng.uniform(0.0, GDN_BOUND, total), rng.uniform(GDN_BOUND, 1.0, total)).astype(np.float32)
    raw[(cls < 2) & (raw >= GDN_BOUND)] = GDN_BOUND / 2      # the float32 rounding of a draw just under the bound
    g_eff = np.abs(n()) + np.float32(1e-3)
    g_eff[cls % 2 == 0] *= -1
    if total >= 255:
        raw[rng.permutation(total)[:16]] = GDN_BOUND
    d["raw"], d["g_eff"] = raw, g_eff
    for v in d.values():
        v.setflags(write=False)
    return d


def reparam_classes(raw, g_eff):
    """Element counts of {raw < bound, raw >= bound} x {g_eff < 0, g_eff > 0}, and of raw == bound."""
    lo, neg = raw < GDN_BOUND, g_eff < 0
    return dict(below_neg=int((lo & neg).sum()), below_pos=int((lo & (g_eff > 0)).sum()), above_neg=int((~lo & neg).sum()),
                above_pos=int((~lo & (g_eff > 0)).sum()), at_bound=int((raw == GDN_BOUND).sum()))


LEAKY = 0.2          # the kernels hold 0.2f, i.e. 0.2 rounded once: that rounding is counted in r


def act_backward_ref(g, y, act):
    """-> (ref, r, S); r == 0: an exact selection, to be compared with ==."""
    g, y = f64(g), f64(y)
    if act == "none":
        return g, 0, None
    if act == "relu":
        return g * (y > 0), 0, None
    if act == "leaky_relu":
        ref = g * np.where(y > 0, 1.0, LEAKY)
        return ref, 2, np.abs(ref)                     # the constant 0.2f, the product
    ref = g * (y * (1.0 - y))
    return ref, 3, np.abs(ref)                         # 1 - y, y (1 - y), g d


def gate_forward_ref(x, t, s):
    x, t, s = f64(x), f64(t), f64(s)
    return x + t * s, 2, np.abs(x) + np.abs(t * s)     # t s, the sum


def gate_backward_ref(g, t, s):
    g, t, s = f64(g), f64(t), f64(s)
    g_t, g_s = g * s, g * t * s * (1.0 - s)
    return (g_t, 1, np.abs(g_t)), (g_s, 4, np.abs(g_s))      # g s | g t, (g t) s, 1 - s, the last product


def axpy_ref(a, b, alpha):
    a, b = f64(a), f64(b)
    return a + alpha * b, 2, np.abs(a) + np.abs(alpha * b)   # alpha b, the sum (alpha itself is a float32 value)


def noise_add_ref(x, noise):
    x, noise = f64(x), f64(noise)
    return x + noise, 1, np.abs(x) + np.abs(noise)


def gdn_apply_ref(x, norm, inverse):
    ref = f64(x) * f64(norm) if inverse else f64(x) / f64(norm)
    return ref, 1, np.abs(ref)                         # one product or one correctly rounded quotient


def gdn_prep_ref(g, x, norm, inverse):
    """-> (q, r, S), |x| (exact)"""
    g, x, n = f64(g), f64(x), f64(norm)
    q = g * x if inverse else -g * x / (n * n)
    return (q, 1 if inverse else 3, np.abs(q)), np.abs(x)    # g x | g x, n n, the quotient


def gdn_finish_ref(g, x, norm, t, inverse):
    g, x, n, t = f64(g), f64(x), f64(norm), f64(t)
    first = g * n if inverse else g / n
    sgn = np.sign(x)                                   # 0 at +0.0 and at -0.0, as torch.abs' gradient
    return first + sgn * t, 2, np.abs(first) + np.abs(sgn * t)     # g n (or g / n), the sum; sign(x) t is exact


def reparam_forward_ref(raw):
    r = np.maximum(f64(raw), float(GDN_BOUND))
    return r * r - float(GDN_PEDESTAL), 2, r * r + float(GDN_PEDESTAL)      # r r, the difference


def reparam_effective(raw_t):
    """tfc.GDNParameter with lower_bound's gradient rule ("identity_if_towards", train_ref._BoundTowards)."""
    return train_ref._BoundTowards.apply(raw_t, float(GDN_BOUND), math.inf) ** 2 - float(GDN_PEDESTAL)


def reparam_backward_ref(raw, g_eff):
    raw_t = torch.tensor(f64(raw), requires_grad=True)
    reparam_effective(raw_t).backward(torch.tensor(f64(g_eff)))
    ref = raw_t.grad.numpy()
    return ref, 1, np.abs(ref)                         # 2 g_eff is exact; one product with max(raw, bound)


TRANSPOSE_CASES = [(25, 33, 48), (1, 3, 5), (81, 96, 140)]       # taps, A, B; the last is past two trips of the grid


# ---- 2. sntc_small_matmul ------------------------------------------------------------------------------------------------
MATMUL_CASES = [(25, 25, TR_CAP + 259), (81, 81, 1031), (1, 1, 1), (96, 128, 300)]      # rows, k, cols; 96 x 128 floats = 48 KB
MATMUL_REFUSED = (97, 128, 8)


@functools.lru_cache(maxsize=None)
def matmul_case(rows, k, cols, transpose_a):
    rng = np.random.default_rng(rows * 1000 + k + cols % 97 + transpose_a)
    a = rng.standard_normal((k, rows) if transpose_a else (rows, k)).astype(np.float32)
    b = rng.standard_normal((k, cols)).astype(np.float32)
    a64 = f64(a).T if transpose_a else f64(a)
    ref = a64 @ f64(b)
    S = np.abs(a64) @ np.abs(f64(b))
    for v in (a, b, ref, S):
        v.setflags(write=False)
    return dict(a=a, b=b, ref=ref, r=k + 1, S=S)         # k fused multiply-adds: a k-term accumulation


# ---- 3. hidden layer of the two-layer decoders, forward and backward -------------------------------------------------------
TAIL_NPIX = 1031
TAIL_CASES = [(ch, has_res, act) for ch in (12, 24, 48) for has_res in (0, 1) for act in (0, 1, 2, 3, 4)]
TAIL_CAP_CASES = [(12, 1, 1), (12, 1, 4)]               # at npix = the launching function's cap + 259
TAIL_ZEROS = 64


@functools.lru_cache(maxsize=None)
def tail_inputs(ch, has_res, npix):
    rng = np.random.default_rng(ch * 10 + has_res + npix % 89)
    c2 = ch * (2 if has_res else 1)
    t = rng.standard_normal((npix, c2)).astype(np.float32)
    base = np.ascontiguousarray(t[:, :ch])
    t[:, :ch] = _with_zeros(rng, base, TAIL_ZEROS)
    g_h = rng.standard_normal((npix, ch)).astype(np.float32)
    beta = (1.0 + 0.5 * rng.random(ch)).astype(np.float32)
    gamma = (0.1 * np.eye(ch) + 0.02 * rng.random((ch, ch))).astype(np.float32)
    for v in (t, g_h, beta, gamma):
        v.setflags(write=False)
    return dict(t=t, g_h=g_h, beta=beta, gamma=gamma)


def hidden_forward(t, ch, has_res, act, beta, gamma):
    """The hidden layer in float64 torch: h = act(t[:, :ch]) (+ t[:, ch:]); act 0 none, 1 IGDN1, 2 GDN1, 3 relu, 4 leaky_relu."""
    base = t[:, :ch]
    if act in (1, 2):
        h = train_ref.gdn(base.t().reshape(1, ch, -1, 1), beta, gamma, inverse=act == 1).reshape(ch, -1).t()
    else:
        h = train_ref.ACTIVATIONS[{0: "none", 3: "relu", 4: "leaky_relu"}[act]](base)
    return h + t[:, ch:] if has_res else h


@functools.lru_cache(maxsize=None)
def tail_reference(ch, has_res, act, npix):
    """Forward value and d sum(h g_h) / d t with the bars of both kernels."""
    d = tail_inputs(ch, has_res, npix)
    t = torch.tensor(f64(d["t"]), requires_grad=True)
    beta, gamma = torch.tensor(f64(d["beta"])), torch.tensor(f64(d["gamma"]))
    h = hidden_forward(t, ch, has_res, act, beta, gamma)
    (h * torch.tensor(f64(d["g_h"]))).sum().backward()
    x, g = f64(d["t"][:, :ch]), f64(d["g_h"])
    res = np.abs(f64(d["t"][:, ch:])) if has_res else 0.0
    nrm = f64(d["beta"]) + np.abs(x) @ f64(d["gamma"])            # ch + 1 positive terms, each product rounded: r = ch + 2
    gam = np.abs(f64(d["gamma"]))
    sgn = np.abs(np.sign(x))
    if act == 1:
        # forward: norm (ch + 2), x norm (+1), + res (+1)
        fwd = (ch + 4, np.abs(x) * nrm + res)
        # backward: dx_i = g_i n_i + sign(x_i) sum_j (g_j x_j) gamma_ij: the sum has ch terms of two products each (ch + 2), the
        # first term is norm (ch + 2) and a product (+1); the longer of the two and the final sum (+1)
        bwd = (ch + 4, np.abs(g) * nrm + sgn * ((np.abs(g * x)) @ gam.T))
    elif act == 2:
        fwd = (ch + 4, np.abs(x) / nrm + res)                     # norm (ch + 2), the quotient, + res
        # backward: dx_i = g_i / n_i - sign(x_i) sum_j g_j x_j gamma_ij / n_j^2.  n is a sum of positive terms, so its ch + 2
        # roundings are a relative error; n n doubles it and rounds (+1), g x rounds (+1), the quotient (+1): 2 ch + 7 per u_j;
        # u_j gamma_ij (+1) summed over ch terms (+ch), the final sum (+1): 3 ch + 9
        bwd = (3 * ch + 9, np.abs(g) / nrm + sgn * ((np.abs(g * x) / (nrm * nrm)) @ gam.T))
    elif act == 4:
        fwd = (2 + has_res, np.abs(h.detach().numpy() - (f64(d["t"][:, ch:]) if has_res else 0.0)) + res)    # 0.2f, the product, + res
        bwd = (2, np.abs(t.grad.numpy()[:, :ch]))                 # 0.2f, the product
    else:                                                         # none, relu: a copy or a selection; + res rounds once
        fwd = (has_res, np.abs(h.detach().numpy() - (f64(d["t"][:, ch:]) if has_res else 0.0)) + res)
        bwd = (0, None)
    out = dict(h=h.detach().numpy(), g_t=t.grad.numpy(), fwd=fwd, bwd=bwd, abs_x=np.abs(x), gx=g * x)
    for v in (out["h"], out["g_t"], out["abs_x"], out["gx"]):
        v.setflags(write=False)
    return out


# ---- 4. sntc_adam_step ----------------------------------------------------------------------------------------------------
ADAM_N = 2 * SGA_CAP + 259
ADAM_STEPS = (1, 7, 1000)
ADAM_ZEROS = 64
ADAM = dict(lr=float(np.float32(1e-3)), beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-7)),
            grad_scale=float(np.float32(0.37)))      # the float32 values the entry point receives


@functools.lru_cache(maxsize=None)
def adam_inputs():
    rng = np.random.default_rng(77)
    p, g, m = (rng.standard_normal(ADAM_N).astype(np.float32) for _ in range(3))
    m *= np.float32(0.1)
    v = (0.01 * rng.random(ADAM_N)).astype(np.float32)
    still = rng.permutation(ADAM_N)[:ADAM_ZEROS]
    g[still] = m[still] = v[still] = 0.0
    for a in (p, g, m, v, still):
        a.setflags(write=False)
    return dict(p=p, g=g, m=m, v=v, still=still)


@functools.lru_cache(maxsize=None)
def adam_reference(t):
    d = adam_inputs()
    p, g, m, v = (f64(d[k]) for k in "pgmv")
    gs = ADAM["grad_scale"] * g
    b1, b2 = ADAM["beta1"], ADAM["beta2"]
    p1, m1, v1 = train_ref.adam_update(p, gs, m, v, ADAM["lr"], t, beta1=b1, beta2=b2, eps=ADAM["eps"])
    alpha = ADAM["lr"] * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    # 1 - beta is exact in float32 (Sterbenz).  m: g_s (1), (1 - b1) g_s (2), the sum (3)
    S_m = np.abs(b1 * m) + np.abs((1 - b1) * gs)
    # v: g_s enters twice (2 relative), two products (4), the sum (5)
    S_v = np.abs(b2 * v) + (1 - b2) * gs * gs
    # step T = alpha m' / (sqrt(v') + eps): m' 3 (against S_m), alpha rounded to float32 (1), alpha m' (1), v' is a sum of
    # non-negative terms, so its 5 roundings are relative and the root halves them (2.5), the root (1), + eps (1), the
    # quotient (1): 11.5; p - T rounds once more: r = 13 against |p| + alpha S_m / (sqrt(v') + eps)
    S_p = np.abs(p) + alpha * S_m / (np.sqrt(v1) + ADAM["eps"])
    return dict(p=(p1, 13, S_p), m=(m1, 3, S_m), v=(v1, 5, S_v))


# ---- 5. sntc_conv_wgrad ----------------------------------------------------------------------------------------------------
WG_CASES = [  # kind, k, s, cin, cout, n, h, w  ->  P, ksplit, pixels of the last slab, pixels of its last 16-pixel stage (0: full)
    (("conv", 5, 2, 3, 64, 3, 33, 29), (765, 2, 381, 13)),         # scalar gather, Hs 33 != 2 * 17
    (("conv", 5, 2, 32, 96, 3, 33, 29), (765, 2, 381, 13)),        # vector gather, 7 row tiles
    (("sigdown", 5, 2, 3, 32, 3, 33, 29), (765, 2, 381, 13)),      # centred padding, odd size
    (("sigdown", 5, 2, 32, 32, 2, 35, 27), (504, 1, 504, 8)),      # one ragged slab
    (("sigup", 5, 2, 32, 32, 3, 17, 15), (765, 2, 381, 13)),
    (("sigup", 5, 2, 32, 3, 3, 17, 15), (765, 2, 381, 13)),        # 3 channels on the gathered side
    (("convT", 5, 2, 32, 48, 3, 17, 15), (765, 2, 381, 13)),       # 10 row tiles
    (("conv", 3, 1, 33, 160, 3, 17, 19), (969, 2, 473, 9)),        # Cs % 4 != 0 with slabs
    (("conv", 5, 2, 40, 40, 5, 63, 65), (5280, 13, 288, 0)),       # many slabs, Hs 63 != 2 * 32, 64-wide tile on 40 columns
    (("sigdown", 9, 4, 3, 32, 2, 45, 51), (312, 1, 312, 8)),       # stride 4, Hs 45 != 4 * 12
    (("sigup", 9, 4, 32, 3, 2, 12, 13), (312, 1, 312, 8)),
]
WG_IDS = ["-".join(str(v) for v in c) for c, _ in WG_CASES]
WG_KINDS = {"conv": 0, "convT": 1, "sigdown": 2, "sigup": 3}      # sntc.h SNTC_CONV2D .. SNTC_SIGNAL_UP
WG_BK, WG_BM = 16, 128                                           # csrc/wgrad.hip kBK, kBM


def wg_split(kind, k, s, cin, cout, n, h, w):
    """csrc/wgrad.hip wg_geometry + wg_pick_bn + wg_split restated -> dict(Cs, Cd, P, ksplit, pslab, last_slab, last_stage)."""
    if kind in ("conv", "sigdown"):
        Cs, Cd, Hd, Wd = cin, cout, -(-h // s), -(-w // s)
    else:
        Cs, Cd, Hd, Wd = cout, cin, h, w
    M, N = k * k * Cs, Cd
    bn, best = 32, 1 << 60
    for c in (32, 64, 96, 128, 160, 192):
        padded = -(-N // c) * c
        if padded <= best:
            best, bn = padded, c
    tiles = -(-M // WG_BM) * -(-N // bn)
    P = n * Hd * Wd
    chunks = -(-P // WG_BK)
    ks = max(1, -(-1536 // tiles))
    ks = min(ks, max(1, chunks // 24), 256)
    per = -(-chunks // ks) * WG_BK
    ksplit = -(-P // per)
    last = P - (ksplit - 1) * per
    return dict(Cs=Cs, Cd=Cd, Hd=Hd, Wd=Wd, P=P, M=M, N=N, ksplit=ksplit, pslab=per, last_slab=last, last_stage=last % WG_BK)


def wg_stages_straddle(geo):
    """Stages of 16 pixels cross row ends everywhere (Wd % 16 != 0), and image ends: either an image is no whole number of
    stages, or (5 x 32 x 33 = 5 x 66 stages) the slabs start inside images."""
    hw = geo["Hd"] * geo["Wd"]
    return geo["Wd"] % WG_BK != 0 and (hw % WG_BK != 0 or geo["pslab"] % hw != 0)


def wg_forward(kind, x, w, s):
    """The layer in float64 (x NCHW); w in the layer's own kernel layout."""
    return {"conv": train_ref.conv2d, "convT": train_ref.conv2d_transpose, "sigdown": train_ref.signal_conv_down,
            "sigup": train_ref.signal_conv_up}[kind](x, w, None, s)


def wg_kernel_shape(kind, k, cin, cout):
    return (k, k, cout, cin) if kind == "convT" else (k, k, cin, cout)       # SignalConv2D kernels are [k, k, cin, cout] both ways


@functools.lru_cache(maxsize=None)
def wg_case(case):
    kind, k, s, cin, cout, n, h, w = case
    rng = np.random.default_rng(k * 1000 + s * 100 + cin + cout + h)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wshape = wg_kernel_shape(kind, k, cin, cout)
    g = None
    out = []
    for absolute in (False, True):          # d sum(y g) / d w, then the same with |x|, |g|: S of the per-element bar
        wt = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
        y = wg_forward(kind, train_ref.as_input(np.abs(x) if absolute else x), wt, s)
        if g is None:
            g = rng.standard_normal((n, y.shape[2], y.shape[3], cout)).astype(np.float32)
        (y * train_ref.as_input(np.abs(g) if absolute else g)).sum().backward()
        out.append(wt.grad.numpy())
    for v in (x, g, out[0], out[1]):
        v.setflags(write=False)
    return dict(x=x, g=g, dw=out[0], S=out[1], shape=wshape)


# ---- 6. sntc_bias_grad ------------------------------------------------------------------------------------------------------
BIAS_CASES = [  # (npix, c) -> pixel slabs (csrc/wgrad.hip bias_slabs)
    ((765, 3), 3), ((969, 33), 4), ((1000, 100), 4), ((5280, 192), 21), ((1, 64), 1)]


def bias_slabs(npix, c):
    strips = -(-c // 64)
    return max(1, min(-(-2048 // strips), -(-npix // 256)))


@functools.lru_cache(maxsize=None)
def bias_case(npix, c):
    g = np.random.default_rng(npix + c).standard_normal((npix, c)).astype(np.float32)
    ref, S = f64(g).sum(0), np.abs(f64(g)).sum(0)
    for v in (g, ref, S):
        v.setflags(write=False)
    return dict(g=g, ref=ref, S=S)


# ---- 7. deep-factorized prior gradients ------------------------------------------------------------------------------------------
PRIOR_CASES = [(c, n, hw) for c in (32, 100, 192) for (n, hw) in ((1, 3), (2, 513))] + [(192, 2, 700)]      # n hw = 3, 1026, 1400
PRIOR_FILTERS = (3, 3)


@functools.lru_cache(maxsize=None)
def prior_params(c):
    """tfc.DeepFactorized variables with matrices and factors away from zero (as tests/test_hip_train.py::_small_model)."""
    rng = np.random.default_rng(c)
    filters = (1,) + PRIOR_FILTERS + (1,)
    scale = 10.0 ** (1.0 / (len(PRIOR_FILTERS) + 1))
    mats, biases, factors = [], [], []
    for k in range(len(filters) - 1):
        fo, fi = filters[k + 1], filters[k]
        init = math.log(math.expm1(1.0 / scale / fo))
        mats.append((init + 0.3 * rng.standard_normal((c, fo, fi))).astype(np.float32))
        biases.append(rng.uniform(-0.5, 0.5, (c, fo)).astype(np.float32))
        if k < len(filters) - 2:
            factors.append((0.3 * rng.standard_normal((c, fo))).astype(np.float32))
    for v in mats + biases + factors:
        v.setflags(write=False)
    return mats, biases, factors


def prior_bits(z, mats, biases, factors):
    """bits per element of z [..., C] (float64 tensors; the reference's parameter shapes [C, fo, fi], [C, fo], [C, fo])."""
    return train_ref.noisy_deep_factorized_bits(z, mats, biases, factors)


@functools.lru_cache(maxsize=None)
def prior_case(c, n, hw):
    mats, biases, factors = prior_params(c)
    rng = np.random.default_rng(c * 7 + n * hw)
    z = (2.0 * rng.standard_normal((n, hw, 1, c))).astype(np.float32)
    zt = torch.tensor(f64(z), requires_grad=True)
    leaves = [[torch.tensor(f64(a), requires_grad=True) for a in grp] for grp in (mats, biases, factors)]
    bits = prior_bits(zt, *leaves)
    bits.sum().backward()
    cat = lambda grp: np.concatenate([t.grad.numpy().ravel() for t in grp])
    out = dict(z=z, bits=bits.detach().numpy().sum(axis=(1, 2, 3)), dz=zt.grad.numpy(), gm=cat(leaves[0]), gb=cat(leaves[1]),
               gf=cat(leaves[2]))
    for v in out.values():
        v.setflags(write=False)
    return out
