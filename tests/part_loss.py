"""Reference arithmetic for the fused training losses (csrc/losses.hip, fused.part_loss); test infrastructure, no GPU.

  * a float32 numpy mirror of the kernel's per-element arithmetic: every numpy float32 operation rounds once, and the
    operations are written in the kernel's order, so elementwise results (the pixel and symmetry gradients) compare bit
    for bit; sums are taken in float64, as the kernel accumulates in double;
  * the same formulas in float64 (the functions below take a dtype), and the losses written with torch in float64 under
    CPU autograd, which the closed-form gradients are checked against;
  * the error bounds of the GPU tests, derived by counting roundings (u = 2^-24 is the unit roundoff of float32).

The losses, in the project's own words (x: a diff, f: a flow pair's member, I: its image, e2 = float32(eps * eps)):
  pixel   = mean sqrt(x^2 + e2)                       or, neg_psnr: mean_b(-log(1 / l_b)) / 100, l_b the mean of sample b
  tv(f,I) = mean over b, y < H-1, x < W-1 of w (T_0 + T_1),  T_c = sqrt(dy_c^2 + dx_c^2 + e2), dy = f(y,x) - f(y+1,x),
            dx = f(y,x) - f(y,x+1),  w = exp(-sum_channels(|I(y,x) - I(y+1,x)| + |I(y,x) - I(y,x+1)|))
  offset  = tv(f0, I0) + tv(f1, I1)
  sym     = mean sqrt((f0 + f1)^2 + e2)
"""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24

# work decomposition of csrc/losses.hip (tests/test_part_loss_host.py checks them against the source)
THREADS = 256
DIFF_BLOCK_UNITS = 1024         # units of 4 elements per diff workgroup
FLOW_BLOCK_UNITS = 256          # units of 4 pixels per flow workgroup
FINISH_THREADS = 256            # partials one pass of the finish workgroup takes


def e2_of(eps, dtype=f32):
    return dtype(f64(eps) * f64(eps))


def charbonnier(x, e2):
    """sqrt(x^2 + e2): square, add, sqrt -- one rounding each in x's dtype"""
    t = x * x
    t = t + e2
    return np.sqrt(t)


def diff_of(d, target):
    return d if target is None else d - target


def partial_counts(B, C, H, W):
    """(diff partials per tensor and sample, flow partials per sample)"""
    units = (W + 3) // 4
    return -(-(C * H * units) // DIFF_BLOCK_UNITS), -(-(H * units) // FLOW_BLOCK_UNITS)


# ------------------------------------------------------------------ forward values

def tv_cells(f, img, e2):
    """per cell (b, y < H-1, x < W-1), in f's dtype and the kernel's order: w, T[c], dy[c], dx[c], exponent A"""
    dt = f.dtype.type
    c0 = img[:, :, :-1, :-1]
    A = np.zeros((img.shape[0], img.shape[2] - 1, img.shape[3] - 1), dt)
    for c in range(img.shape[1]):                           # channels in order
        edge = np.abs(c0[:, c] - img[:, c, 1:, :-1]) + np.abs(c0[:, c] - img[:, c, :-1, 1:])
        A = A + edge
    w = np.exp(-A)
    dy = f[:, :, :-1, :-1] - f[:, :, 1:, :-1]
    dx = f[:, :, :-1, :-1] - f[:, :, :-1, 1:]
    t = dy * dy + dx * dx
    t = t + dt(e2)
    T = np.sqrt(t)
    return w, T, dy, dx, A


def values(diffs, target, flows, images, eps, neg_psnr, dtype=f32):
    """(values[nd + 2], sample_means[nd, B]): terms in `dtype`, sums in float64, the results rounded to dtype as the
    finish kernel rounds them"""
    dt = dtype
    e2 = e2_of(eps, dt)
    vals, means = [], []
    tgt = None if target is None else target.astype(dt)
    for d in diffs:
        x = diff_of(d.astype(dt), tgt)
        s = charbonnier(x, e2).astype(f64)
        l = (s.reshape(s.shape[0], -1).sum(1) / f64(s[0].size)).astype(dt)
        means.append(l)
        if neg_psnr:
            v = -np.log(dt(1.0) / l) / dt(100.0)
            vals.append(dt(v.astype(f64).sum() / len(l)))
        else:
            vals.append(dt(s.sum() / f64(s.size)))
    if flows is None:
        vals += [dt(0.0), dt(0.0)]
    else:
        tvs = []
        for f, img in zip(flows, images):
            w, T, _, _, _ = tv_cells(f.astype(dt), img.astype(dt), e2)
            term = w * (T[:, 0] + T[:, 1])
            tvs.append(dt(term.astype(f64).sum() / f64(term.size)))
        vals.append(tvs[0] + tvs[1])
        s = charbonnier(flows[0].astype(dt) + flows[1].astype(dt), e2).astype(f64)
        vals.append(dt(s.sum() / f64(s.size)))
    return np.array(vals, dt), np.array(means, dt)


# ------------------------------------------------------------------ gradients, closed form

def pixel_grad(d, target, g, eps, neg_psnr, sample_means=None, dtype=f32):
    """gradient of g * pixel with respect to d (the network output when target is given), the kernel's operations in order"""
    dt = dtype
    e2 = e2_of(eps, dt)
    x = diff_of(d.astype(dt), None if target is None else target.astype(dt))
    B = x.shape[0]
    ratio = x / charbonnier(x, e2)
    if neg_psnr:
        coef = (dt(g) / dt(100 * B)) / sample_means.astype(dt)
        coef = coef / dt(x[0].size)
        return coef.reshape(B, 1, 1, 1) * ratio
    return (dt(g) / dt(x.size)) * ratio


def sym_grad(f0, f1, g, eps, dtype=f32):
    """gradient of g * sym with respect to f0 (= that with respect to f1)"""
    dt = dtype
    u = f0.astype(dt) + f1.astype(dt)
    return (dt(g) / dt(u.size)) * (u / charbonnier(u, e2_of(eps, dt)))


def tv_grad_terms(f, img, g, eps, dtype=f32):
    """the three total-variation terms of the gradient of g * tv(f, img) with respect to f, each [B,2,H,W] (0 where the
    cell does not exist), in the kernel's operations: own, up (cell (y-1,x)), left (cell (y,x-1)); and the magnitudes
    M >= |term| the error bound is stated in (the same products with |dy| + |dx|, |dy|, |dx| for the numerators)"""
    dt = dtype
    f = f.astype(dt)
    B, _, H, W = f.shape
    w, T, dy, dx, _ = tv_cells(f, img.astype(dt), e2_of(eps, dt))
    k = dt(g) / dt(B * (H - 1) * (W - 1))
    kw = (k * w)[:, None]
    own, up, left = (np.zeros(f.shape, dt) for _ in range(3))
    own[:, :, :-1, :-1] = kw * ((dy + dx) / T)
    up[:, :, 1:, :-1] = kw * (dy / T)
    left[:, :, :-1, 1:] = kw * (dx / T)
    mags = [np.zeros(f.shape, f64) for _ in range(3)]
    akw = np.abs(kw.astype(f64))
    mags[0][:, :, :-1, :-1] = akw * (np.abs(dy) + np.abs(dx)) / T
    mags[1][:, :, 1:, :-1] = akw * np.abs(dy) / T
    mags[2][:, :, :-1, 1:] = akw * np.abs(dx) / T
    return (own, up, left), mags


def flow_grad(f, other, img, g_tv, g_sym, eps, dtype=f32):
    """the flow gradient as the kernel adds it: 0 + own - up - left + sym (absent terms skipped); g_tv / g_sym None = the
    loss is unused"""
    dt = dtype
    acc = np.zeros(f.shape, dt)
    if g_tv is not None:
        (own, up, left), _ = tv_grad_terms(f, img, g_tv, eps, dt)
        acc = acc + own
        acc = acc - up
        acc = acc - left
    if g_sym is not None:
        acc = acc + sym_grad(f, other, g_sym, eps, dt)
    return acc


# ------------------------------------------------------------------ float64 under torch autograd

def torch_losses(diffs, target, flows, images, eps, neg_psnr):
    """the losses written with torch operations on float64 tensors: (pixel list, offset or None, sym or None)"""
    import torch
    e2 = float(e2_of(eps, f64))

    def charb(x):
        return torch.sqrt(x * x + e2)

    pixel = []
    for d in diffs:
        x = d if target is None else d - target
        if neg_psnr:
            l = charb(x).flatten(1).mean(1)
            pixel.append(torch.mean(-torch.log(1.0 / l) / 100.0))
        else:
            pixel.append(charb(x).mean())
    if flows is None:
        return pixel, None, None

    def tv(f, img):
        c0 = img[:, :, :-1, :-1]
        w = torch.exp(-((c0 - img[:, :, 1:, :-1]).abs() + (c0 - img[:, :, :-1, 1:]).abs()).sum(1))
        f00 = f[:, :, :-1, :-1]
        T = torch.sqrt((f00 - f[:, :, 1:, :-1]) ** 2 + (f00 - f[:, :, :-1, 1:]) ** 2 + e2).sum(1)
        return (w * T).mean()

    return pixel, tv(flows[0], images[0]) + tv(flows[1], images[1]), charb(flows[0] + flows[1]).mean()


def reference64(diffs, target, flows, images, eps, neg_psnr, grad_values=None):
    """float64: values[nd + 2]; with grad_values also the gradients of sum_j grad_values[j] * values[j] with respect to
    every diff and both flows (torch CPU autograd)"""
    import torch
    t64 = lambda a, grad=False: torch.from_numpy(np.ascontiguousarray(a, dtype=f64)).requires_grad_(grad)   # noqa: E731
    want = grad_values is not None
    td = [t64(d, want) for d in diffs]
    tf = None if flows is None else [t64(f, want) for f in flows]
    ti = None if flows is None else [t64(i) for i in images]
    pixel, offset, sym = torch_losses(td, None if target is None else t64(target), tf, ti, eps, neg_psnr)
    zero = torch.zeros((), dtype=torch.float64)
    vals = pixel + [zero if offset is None else offset, zero if sym is None else sym]
    out = np.array([float(v.detach()) for v in vals], f64)
    if not want:
        return out
    total = sum(float(g) * v for g, v in zip(grad_values, vals) if v.requires_grad)
    total.backward()
    zeros = lambda t: np.zeros(tuple(t.shape), f64)                     # noqa: E731
    gd = [zeros(t) if t.grad is None else t.grad.numpy() for t in td]
    gf = None if tf is None else [zeros(t) if t.grad is None else t.grad.numpy() for t in tf]
    return out, gd, gf


# ------------------------------------------------------------------ bounds (u = 2^-24)

# One Charbonnier term sqrt(x^2 + e2), relative: the subtraction out - target <= 1 (d term / d x * x / term <= 1), the
# square 1/2 and the add 1/2 (both under the square root), the sqrt 1: 3.  The sum in double and the division by n add
# less than one more (n 2^-53), the final rounding to float32 one: K = 5, and 6 leaves room for the second-order terms.
# The symmetry term has the same count with f0 + f1 in place of the subtraction.
K_PIXEL = 6
K_SYM = 6


def k_tv(ci, amax):
    """One total-variation term w (T_0 + T_1), relative: T_c as above with two subtractions sharing the weight of one (1),
    two squares (1/2), two adds (1/2 + 1/2) and the sqrt (1): 3.5; T_0 + T_1: 1; the product with w: 1; expf: 1 ulp in the
    ROCm math library's table = 2 u; the exponent's absolute error is the relative error of w: its 2 ci subtractions add up
    to u A and each of the 2 ci - 1 additions rounds a partial sum <= A, so <= 2 ci u A with A <= amax = 2 ci max|dI|;
    the double sum < 1, the mean's rounding 1, the add of the two means 1: 11 + 2 ci amax."""
    return 11.0 + 2.0 * ci * amax


def value_bounds(ref, diffs, target, flows, images, eps, neg_psnr):
    """|v - ref| <= bound, per value, from the float64 reference and the inputs alone"""
    nd = len(diffs)
    bound = np.zeros(nd + 2)
    for i, d in enumerate(diffs):
        if not neg_psnr:
            bound[i] = K_PIXEL * U * abs(ref[i])
            continue
        # per sample v_b = -log(1 / l_b) / 100: l_b carries (K_PIXEL) u relative = that much absolute in the logarithm; the
        # reciprocal one more; logf 1 ulp = 2 u of |log|, the negation none, the division 1 u of |log|: then the mean of the
        # samples (double) and its rounding, 1 u of |ref|
        x = diff_of(d.astype(f64), None if target is None else target.astype(f64))
        l = charbonnier(x, e2_of(eps, f64)).reshape(x.shape[0], -1).mean(1)
        bound[i] = U * (np.mean((K_PIXEL + 1) + 3 * np.abs(np.log(l))) / 100.0 + abs(ref[i]))
    if flows is not None:
        ci = images[0].shape[1]
        amax = max(float(tv_cells(f.astype(f64), i.astype(f64), 0.0)[4].max()) for f, i in zip(flows, images))
        bound[nd] = k_tv(ci, amax) * U * abs(ref[nd])
        bound[nd + 1] = K_SYM * U * abs(ref[nd + 1])
    return bound


def flow_grad_bound(f, other, img, g_tv, g_sym, eps):
    """|grad - ref| <= bound per element of the flow gradient: the sum of the bounds of its (at most four) terms, which can
    cancel.  A total-variation term (k w) (num / T) with magnitude M = |k w| (|dy| + |dx|) / T (own; |dy| or |dx| alone for
    up and left): the differences 1, their sum 1, T 3.5, the division 1, k = g / float(n) 2, w 2 + 2 ci amax (k_tv's
    docstring), k w 1, the last product 1: (12.5 + 2 ci amax) u M, taken as 14 + 2 ci amax.  The symmetry term
    ks (u / s): the sum 1, s 2 (square, add under the root, sqrt), the division 1, ks 2, the product 1: 7 u M_sym.  Adding
    the terms rounds at most three partial sums, each <= the sum of the magnitudes."""
    total = np.zeros(f.shape, f64)
    bound = np.zeros(f.shape, f64)
    if g_tv is not None:
        _, mags = tv_grad_terms(f, img, g_tv, eps, f64)
        amax = float(tv_cells(f.astype(f64), img.astype(f64), 0.0)[4].max())
        for m in mags:
            bound += (14.0 + 2.0 * img.shape[1] * amax) * m
            total += m
    if g_sym is not None:
        m = np.abs(sym_grad(f, other, g_sym, eps, f64))
        bound += 7.0 * m
        total += m
    return U * (bound + 3.0 * total)
