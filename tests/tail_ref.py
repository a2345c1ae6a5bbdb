"""fp64 restatements of the small kernels around the fused chains -- csrc/geo.hip, the positional encoding and the background
head of csrc/render.hip, csrc/loss.hip -- written from the reference's Python lines that the kernels' comments cite, on the
CPU in torch float64.  Each takes the fp32 inputs the kernel gets and upcasts them, so a difference is the kernel's own
rounding (or a wrong index).  Where a per-element bound needs it, a function also returns the magnitude the rounding errors
scale with: the sum of the absolute values of the terms that are added (equal to |result| where nothing cancels).

Also here: the table of "wrapping" shapes of the kernels that walk t, t + stride, ... with at most 8192 blocks of 256 threads
(`geo_blocks`, the same cap in render.hip), and an integer emulation of `RowCol` (csrc/common.h) that the CPU tests use to
show that each shape really takes later passes and the carry."""
import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of fp32
FLT_MIN = 2.0 ** -126               # smallest normal fp32
STRIDE = 8192 * 256                 # threads of a capped launch: the distance between two elements of one thread
F64 = torch.float64


def d(t):
    return t.detach().cpu().to(F64)


# ---- csrc/geo.hip ------------------------------------------------------------------------------------------------------------
def _bands(M):
    return 2.0 ** torch.arange(M, dtype=F64)


def encode(x, M, segs=()):
    """python/network.py:96-117, 154-170: [x | cos(x_d 2^k) (d major, k fastest) | sin(...) | segments...].  x 2^k is exact in
    fp32, so the fp64 value at the fp32 x has no argument error."""
    x = d(x)
    b = (x.unsqueeze(-1) * _bands(M)).reshape(x.shape[0], -1)
    return torch.cat([x, torch.cos(b), torch.sin(b)] + [d(s) for s in segs], dim=-1)


def normal_from_g0(e, g0, M, gqs=()):
    """python/renderer.py:52 (`nn.grad([sdf], [x])`) for the encoding above: n = g0[:, :3] + sum_k 2^k (g_sin cos - g_cos sin)
    + sum_i gq_i, the cos / sin read from the given e.  -> (n, sum of |terms|, number of terms)."""
    e, g0 = d(e), d(g0)
    P = e.shape[0]
    cosb, sinb = e[:, 3:3 + 3 * M].reshape(P, 3, M), e[:, 3 + 3 * M:3 + 6 * M].reshape(P, 3, M)
    gc, gs = g0[:, 3:3 + 3 * M].reshape(P, 3, M), g0[:, 3 + 3 * M:3 + 6 * M].reshape(P, 3, M)
    terms = [g0[:, :3]] + [d(q) for q in gqs]
    if M:
        bands = _bands(M)
        terms += list((gs * cosb * bands).unbind(-1)) + list((-gc * sinb * bands).unbind(-1))
    return sum(terms), sum(t.abs() for t in terms), len(terms)


def gbar0(e, nbar, M, segs=()):
    """g-bar_0 = J_e(x) n-bar: [nbar | -sin(b) nbar_d 2^k | cos(b) nbar_d 2^k | segments...] (cos / sin read from e)."""
    e, nbar = d(e), d(nbar)
    P = e.shape[0]
    cosb, sinb = e[:, 3:3 + 3 * M].reshape(P, 3, M), e[:, 3 + 3 * M:3 + 6 * M].reshape(P, 3, M)
    nb = nbar.unsqueeze(-1) * _bands(M)
    return torch.cat([nbar, (-sinb * nb).reshape(P, -1), (cosb * nb).reshape(P, -1)] + [d(s) for s in segs], dim=-1)


def backward_begin(P, D, g_sdf, g_feat, g_n, gZ):
    """gy = [g_sdf | g_feat + gZ[:, 3:3+D]], nbar = g_n + gZ[:, 3+D:6+D]; an absent term is zero."""
    z = lambda *s: torch.zeros(*s, dtype=F64)
    gy = torch.cat([d(g_sdf).reshape(P, 1) if g_sdf is not None else z(P, 1),
                    (d(g_feat)[:, :D] if g_feat is not None else z(P, D)) + (d(gZ)[:, 3:3 + D] if gZ is not None else z(P, D))], dim=-1)
    nbar = (d(g_n) if g_n is not None else z(P, 3)) + (d(gZ)[:, 3 + D:6 + D] if gZ is not None else z(P, 3))
    return gy, nbar


def inverse_squared_distance(x, camloc, rows_per_batch):
    """python/network.py:405-409: 1 / (F.norm(x - camloc)**2 + 1e-5), the square of the root; row p belongs to camera
    p // rows_per_batch."""
    x, cam = d(x)[:, :3], d(camloc)
    b = torch.arange(x.shape[0]) // rows_per_batch
    nrm = torch.sqrt(((x - cam[b]) ** 2).sum(-1))
    return 1.0 / (nrm ** 2 + float(np.float32(1e-5)))


# ---- csrc/render.hip: positional encoding, background head ----------------------------------------------------------------------
def posenc(x, M, include_input):
    """python/network.py:96-117 for any channel count: [x | cos(x_i 2^k) (i major, k fastest) | sin(...)]."""
    x = d(x).reshape(-1, x.shape[-1])
    b = (x.unsqueeze(-1) * _bands(M)).reshape(x.shape[0], -1)
    return torch.cat(([x] if include_input else []) + [torch.cos(b), torch.sin(b)], dim=-1)


def posenc_backward(x, g, M, include_input):
    """gx_i = g_x_i + sum_k 2^k (-sin(b) g_cos + cos(b) g_sin).  -> (gx, sum of |terms|, number of terms)."""
    x = d(x).reshape(-1, x.shape[-1])
    P, C = x.shape
    g = d(g).reshape(P, -1)
    off = C if include_input else 0
    bands = _bands(M)
    b = x.unsqueeze(-1) * bands
    gc, gs = g[:, off:off + C * M].reshape(P, C, M), g[:, off + C * M:].reshape(P, C, M)
    terms = ([g[:, :C]] if include_input else []) + list((-torch.sin(b) * gc * bands).unbind(-1)) + list((torch.cos(b) * gs * bands).unbind(-1))
    if not terms:
        return torch.zeros(P, C, dtype=F64), torch.zeros(P, C, dtype=F64), 0
    return sum(terms), sum(t.abs() for t in terms), len(terms)


def softplus100(v):
    """F.softplus with beta = 100 and its threshold 20: linear where 100 v > 20."""
    return torch.where(100.0 * v > 20.0, v, torch.log1p(torch.exp(torch.clamp(100.0 * v, max=20.0))) / 100.0)


def background_head(h, x, delta):
    """python/network.py:543-556: alpha = 1 - exp(-softplus_100(h_0) delta), input of the lighting net [x | h_1..F]."""
    h, x, delta = d(h), d(x), d(delta)
    alpha = 1.0 - torch.exp(-softplus100(h[..., 0:1]) * delta)
    return alpha, torch.cat([x, h[..., 1:]], dim=-1)


def background_head_backward(h, delta, g_alpha, g_inp, nx):
    """d/dh of the above; an absent upstream gradient is zero."""
    h, delta = d(h), d(delta)
    g_h = torch.zeros_like(h)
    if g_inp is not None:
        g_h[..., 1:] = d(g_inp)[..., nx:]
    if g_alpha is not None:
        v = h[..., 0:1]
        dsoft = torch.where(100.0 * v > 20.0, torch.ones_like(v), torch.sigmoid(100.0 * v))
        g_h[..., 0:1] = d(g_alpha) * delta * torch.exp(-softplus100(v) * delta) * dsoft
    return g_h


# ---- csrc/loss.hip ---------------------------------------------------------------------------------------------------------------
def pixel_normal(g, eps):
    """python/renderer.py:90-91: n = (g + eps) / |g + eps|.  The fp32 sum g + eps is the kernel's first operation and the
    reference's too; it is taken in fp32 here so that a row of -eps is the same 0 / 0."""
    v = d(g.detach().float() + float(eps))
    return v / torch.sqrt((v * v).sum(-1, keepdim=True))


def pixel_normal_backward(g, eps, gn):
    """(gn - n (n . gn)) / len.  -> (gg, sum of |terms|)."""
    v = d(g.detach().float() + float(eps))
    gn = d(gn)
    ln = torch.sqrt((v * v).sum(-1, keepdim=True))
    n = v / ln
    dot_terms = n * gn
    return (gn - n * dot_terms.sum(-1, keepdim=True)) / ln, (gn.abs() + n.abs() * dot_terms.abs().sum(-1, keepdim=True)) / ln


def pixel_compose(pix, env, spec, bg, entangle, g=None):
    """python/renderer.py:163-178: diffuse = env + implicit; color = base diffuse + photo spec (entangle) or
    photo (base diffuse + spec); + background.  With g: also the gradients [pix, env, spec(, bg)] and, per gradient, the sum of
    |terms| of its element (autograd of the same expression with every factor replaced by its absolute value)."""
    def f(pix, env, spec, bg):
        imp, photo, base = pix[..., 0:1], pix[..., 5:6], pix[..., 6:9]
        diff = env + imp
        fg = base * diff + photo * spec if entangle else photo * (base * diff + spec)
        return fg + bg if bg is not None else fg
    ins = [d(t).requires_grad_(True) for t in (pix, env, spec)] + ([d(bg).requires_grad_(True)] if bg is not None else [])
    color = f(*ins, *(() if bg is not None else (None,)))
    if g is None:
        return color.detach()
    grads = torch.autograd.grad(color, ins, d(g))
    # magnitudes: every product of the backward pass with absolute factors; diffuse = |env| + |implicit| bounds |env + implicit|
    ab = [d(t).abs().requires_grad_(True) for t in (pix, env, spec)] + ([d(bg).abs().requires_grad_(True)] if bg is not None else [])
    mags = torch.autograd.grad(f(*ab, *(() if bg is not None else (None,))), ab, d(g).abs())
    return color.detach(), list(grads), list(mags)


LOSS_TERM_NAMES = ("loss", "loss_rgb", "loss_eikonal", "loss_tv", "prior_base_color", "prior_roughness", "reg_std_roughness",
                   "prior_specular_reflectance", "reg_std_specular_reflectance")


def loss_terms(color, color_gt, mask, grad_x, prior, tvs, N, inv_rays, weights, l2, N_prior=None, mask_sum_global=None,
               upstream=1.0):
    """python/loss.py:59-178 without the mask term.  color, color_gt (B,R,3); mask (B,R,1,1), any real values; grad_x (B,R,N,3)
    or None; prior (B,R,5) per-ray sums [base colour, roughness, log std roughness, specular, log std specular] or None; tvs:
    list of (B,R,N,D) sampled TV tensors.  weights = (eikonal, tv, base colour, roughness, specular): a term whose weight is
    zero is not evaluated (python/loss.py:70, 85, 124, 135, 152) -- it is reported as 0, stays out of the total, and no
    gradient flows to its inputs.  Every term but the RGB one is divided by sum(mask) N + 1e-5 (the priors: N_prior), with
    sum(mask) = mask_sum_global where given.
    -> dict(terms={name: float}, inv_denorm, inv_denorm_prior, grads=dict(color, grad_x, prior, tvs) of `upstream` x d total,
    gx_mag = the magnitude |d total / d grad_x| would have with (|grad| + 1) in place of (|grad| - 1): the difference cancels)."""
    w_e, w_tv, w_bc, w_r, w_s = [float(w) for w in weights]
    N_prior = N if N_prior is None else N_prior
    leaf = lambda t: None if t is None else d(t).requires_grad_(True)
    color, grad_x, prior = leaf(color), leaf(grad_x), leaf(prior)
    tvs = [leaf(t) for t in tvs]
    gt, mask = d(color_gt), d(mask)
    B, R = color.shape[:2]
    eps = float(np.float32(1e-5))
    msum = mask.sum() if mask_sum_global is None else d(mask_sum_global).reshape(())
    denorm, dprior = msum * N + eps, msum * N_prior + eps
    zero = torch.zeros((), dtype=F64)
    diff = color - gt
    l_rgb = ((diff ** 2) if l2 else diff.abs()).sum() * float(inv_rays)
    l_eik = l_tv = zero
    p = [zero] * 5
    if w_e > 0.0 and grad_x is not None:
        gn = torch.sqrt((grad_x * grad_x).sum(-1, keepdim=True))
        l_eik = (((gn - 1.0) * mask) ** 2).sum() / denorm
    if w_tv > 0.0:
        for t in tvs:
            l_tv = l_tv + (t * mask).sum() / denorm
    if prior is not None:
        pm = lambda k: (prior[..., k] * mask.reshape(B, R)).sum() / dprior
        if w_bc > 0.0:
            p[0] = pm(0)
        if w_r > 0.0:
            p[1], p[2] = pm(1), pm(2)
        if w_s > 0.0:
            p[3], p[4] = pm(3), pm(4)
    total = l_rgb
    for w, t in ((w_e, l_eik), (w_tv, l_tv), (w_bc, p[0]), (w_r, p[1]), (w_s, p[3]), (w_r, p[2]), (w_s, p[4])):
        if w > 0.0:
            total = total + w * t
    terms = dict(zip(LOSS_TERM_NAMES, [total, l_rgb, l_eik, l_tv] + p))
    leaves = [color] + [t for t in [grad_x, prior] + tvs if t is not None]
    got = list(torch.autograd.grad(total, leaves, torch.tensor(float(upstream), dtype=F64), allow_unused=True))
    got = [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves)]
    grads = dict(color=got.pop(0), grad_x=got.pop(0) if grad_x is not None else None, prior=got.pop(0) if prior is not None else None,
                 tvs=got)
    gx_mag = None
    if grad_x is not None:
        gxd = grad_x.detach()
        gn = torch.sqrt((gxd * gxd).sum(-1, keepdim=True))
        gx_mag = (abs(float(upstream)) * w_e * 2.0 * (gn + 1.0) / gn * mask ** 2 * gxd.abs() / denorm).detach()
    return dict(terms={k: float(v.detach()) for k, v in terms.items()}, inv_denorm=float(1.0 / denorm), inv_denorm_prior=float(1.0 / dprior),
                grads=grads, gx_mag=gx_mag)


# ---- the capped grid-stride walk ---------------------------------------------------------------------------------------------------
# name -> P rows, W work items per row (what RowCol divides by; None: the kernel divides t by a constant), the kernel's
# parameters, and `largest`: floats of the largest array the GPU test allocates for it (row strides included).
WRAP_SHAPES = {
    "geo_encode": dict(P=120001, W=49, M=6, segs=(4, 6), lde=52, largest=120001 * 52),
    "geo_gbar0": dict(P=120001, W=49, M=6, segs=(4, 6), lde=52, largest=120001 * 52),
    "geo_backward_begin": dict(P=500003, W=11, D=7, ldf=9, ldz=16, largest=500003 * 16),
    "geo_backward_begin_v4": dict(P=600001, W=9, D=20, ldf=21, ldz=26, largest=600001 * 26),
    "copy_columns": dict(P=1100003, W=5, lds=7, ldd=6, largest=1100003 * 7),
    "posenc": dict(P=140001, W=39, C=3, M=6, include_input=True, largest=140001 * 39),
    "posenc_backward": dict(P=1750001, W=3, C=3, M=1, include_input=True, largest=1750001 * 9),
    "background_head": dict(P=21001, W=259, nx=3, F=256, largest=21001 * 259),
    "background_head_backward": dict(P=21001, W=257, nx=3, F=256, largest=21001 * 259),
    "geo_normal": dict(P=1750001, W=3, rowcol=False, M=1, lde=9, D=0, ldz=7, largest=1750001 * 9),
    "inverse_squared_distance": dict(P=5300001, W=1, rowcol=False, ldx=3, ldo=2, rows_per_batch=1000003, largest=5300001 * 3),
}


def launch_threads(total):
    """Threads of a capped launch over `total` elements (`geo_blocks`)."""
    blocks = (total + 255) // 256
    return 256 * min(max(blocks, 1), 8192)


def rowcol_walk(P, W):
    """Integer emulation of `RowCol` (csrc/common.h) under the loop `for (t = t0; t < P W; t += stride, rc.next())` of every
    thread t0 of the launch: the constructor's 32-bit branch in uint32 arithmetic, `next()` as written.
    -> (flat indices p W + c in visiting order, per-element t, dq, dr, passes of thread 0, times a carry was taken, times
    the carry was taken at c == W exactly -- the case in which `>=` and `>` differ)."""
    total = P * W
    stride = launch_threads(total)
    assert total <= 0x7fffffff and stride <= 0x7fffffff
    t0 = np.arange(stride, dtype=np.uint32)
    W32 = np.uint32(W)
    q = t0 // W32
    p = q.astype(np.int64)
    c = (t0 - q * W32).astype(np.int32)
    sq = np.uint32(stride) // W32
    dq, dr = int(sq), int(np.uint32(stride) - sq * W32)
    t = t0.astype(np.int64)
    flat, ts, carries, exact, passes = [], [], 0, 0, 0
    while True:
        live = t < total
        if not live.any():
            break
        passes += 1
        assert (c[live] >= 0).all() and (c[live] < W).all(), "a column outside the row"
        flat.append(p[live] * W + c[live])
        ts.append(t[live])
        t = t + stride
        p = p + dq
        c = c + np.int32(dr)
        carry = c >= W
        carries += int((carry & (t < total)).sum())
        exact += int(((c == W) & (t < total)).sum())
        c = np.where(carry, c - np.int32(W), c)
        p = p + carry
    return np.concatenate(flat), np.concatenate(ts), dq, dr, passes, carries, exact
