"""fp64 restatements of the per-ray kernels of csrc/render.hip -- alpha / transmittance / weights, the VR integrals, the light
integrals, the material head and the gain -- written from the reference's Python lines that the kernels' comments cite
(python/renderer.py:55-87, :105-178, python/specular_brdf.py:23-199, python/network.py:229-231, :288-296, :372-376, :456-508,
python/loss.py:117-166), on the CPU in torch.  Each function takes the fp32 inputs the kernel gets, in the kernel's layout (rays
first, no batch axis), and upcasts them; values come from the formulas, gradients from torch.autograd on the same formulas (the
hand-derived backward is the thing under test).  Every reduced quantity comes with the sum of the absolute values of the terms
that are added and their number T.  With `dtype=torch.float32` the same functions are the fp32 stock-op composite that the GPU
tests measure rho32 with.

Also here: the seeded input builders, which keep every kink of these formulas at least `KINK * max(1, |operands|)` away from the
data (a redraw, never an exclusion), and the integer launch geometry of the host code, which the CPU tests use to show that each
shape of tests/test_gpu_rays.py enters the path it is meant for."""
import math

import numpy as np
import torch

from tests.tail_ref import F64, FLT_MIN, U

F32 = torch.float32
KINK = 64 * U                        # margin of the builders
E5 = float(np.float32(1e-5))         # the kernels' 1e-5f
RD_SLOTS, IM_SEGS, SH_THREADS, MH_THREADS = 512, 6, 128, 128


def up(t, dtype=F64):
    return None if t is None else t.detach().cpu().to(dtype)


def f32(v):
    return float(np.float32(v))


# ---- (a) alpha, transmittance, weights (python/renderer.py:55-82) ---------------------------------------------------------------
def alpha_parts(sdf, n, raydir, t, gain, car):
    """renderer.py:56-66 for tensors of one dtype: sdf (R,N), n (R,N,3), raydir (R,3), t (R,N+1), gain broadcastable to (R,N),
    car scalar.  -> dict of every intermediate (q before the clamp, alpha after it)."""
    tc = (raydir[:, None, :] * n).sum(-1)
    P = (raydir[:, None, :] * n).abs().sum(-1)
    a0, a1 = -tc * 0.5 + 0.5, -tc
    ic = -(torch.relu(a0) * (1.0 - car) + torch.relu(a1) * car)
    delta = t[:, 1:] - t[:, :-1]
    s1, s0 = sdf + ic * delta * 0.5, sdf - ic * delta * 0.5
    x0, x1 = gain * s0, gain * s1
    c0, c1 = torch.sigmoid(x0), torch.sigmoid(x1)
    q = (c0 - c1 + E5) / (c0 + E5)
    return dict(tc=tc, P=P, a0=a0, a1=a1, ic=ic, delta=delta, s0=s0, s1=s1, x0=x0, x1=x1, c0=c0, c1=c1, q=q, alpha=q.clamp(0.0, 1.0))


def alpha_roundings(p, gain, car):
    """What the fp32 evaluation of renderer.py:56-66 can be off by, per sample, in units of u |alpha| -- read from `alpha_terms`:
    * tc = d . n carries 3 u P, P = sum_i |d_i n_i|; a relu of iter_cos that is open hands that on, so iter_cos is off by
      rho u |ic| with rho = 3 P |d ic / d tc| / |ic| + 4 (large where -tc / 2 + 1 / 2 has cancelled to little and the other relu
      is shut);
    * x1 = gain (sdf + ic delta / 2) is off by u (2 |x1| + G (1 + rho)), G = gain |ic delta| / 2 -- the relative error of
      sigmoid(-x1); x0 likewise, the relative error of c0 = sigmoid(x0) times sigmoid(-x0) <= 1 (c0 enters numerator and
      denominator: at most once);
    * the argument of expm1f, gain (ic delta), is off by (rho + 3) u relative, and so is 1 - exp of it; expf / expm1f 2 u each;
    * the remaining 9 operations.
    -> 2 |x1| + 2 |x0| sigmoid(-x0) + (2 G + 1) (1 + rho) + 19.  Where iter_cos is 0, rho = G = 0 and this is
    2 |x1| + 2 |x0| sigmoid(-x0) + 20: the 2 |x1| + 15 of test_alpha_far_outside_the_surface_keeps_its_relative_accuracy, c0's
    share and five roundings more; everywhere else rho >= 4."""
    dic = 0.5 * (1.0 - car) * (p["a0"] > 0) + car * (p["a1"] > 0)
    ic = p["ic"].abs()
    rho = torch.where(ic > 0, 3.0 * p["P"] * dic / ic.clamp(min=1e-300) + 4.0, torch.zeros_like(ic))
    G = (gain * p["ic"] * p["delta"]).abs() * 0.5
    return 2 * p["x1"].abs() + 2 * p["x0"].abs() * torch.sigmoid(-p["x0"]) + (2 * G + 1) * (1 + rho) + 19, rho, G


def alpha_fg(sdf, n, raydir, t, gain, car, dtype=F64):
    """-> (alpha_fg (R,N), its bound in units of u |alpha| (`alpha_roundings`))."""
    g, c = up(gain, dtype).reshape(()), up(car, dtype).reshape(())
    p = alpha_parts(up(sdf, dtype), up(n, dtype), up(raydir, dtype), up(t, dtype), g, c)
    return p["alpha"], alpha_roundings(p, g, c)[0]


def alpha_fp32_spelling(sdf, n, raydir, t, gain, car):
    """`alpha_terms` of csrc/render.hip operation by operation in torch float32 on the CPU (sigmoid as 1 / (1 + exp(-x)), the
    difference of the sigmoids as c0 sigmoid(-x1) (-expm1(gain ic delta)), no fused multiply-add): what plain fp32 arithmetic
    gives for this formula, against which a bound on the kernel can be judged without a GPU."""
    sdf, n, rd, t, gain, car = (x.detach().cpu().float() for x in (sdf, n, raydir, t, gain, car))
    tc = (rd[:, None, 0] * n[..., 0] + rd[:, None, 1] * n[..., 1]) + rd[:, None, 2] * n[..., 2]
    ic = -(torch.relu(-tc * 0.5 + 0.5) * (1.0 - car) + torch.relu(-tc) * car)
    delta = t[:, 1:] - t[:, :-1]
    s1, s0 = sdf + ic * delta * 0.5, sdf - ic * delta * 0.5
    sg = lambda x: 1.0 / (1.0 + torch.exp(-x))
    c0 = sg(gain * s0)
    dc = c0 * sg(-gain * s1) * -torch.expm1(gain * (ic * delta))
    return ((dc + 1e-5) / (c0 + 1e-5)).clamp(0.0, 1.0)


def scan(alpha_all, dtype=F64):
    """renderer.py:79-82 given the per-sample alpha (R,S) (the kernel's own fp32 alpha_fg times mask, then alpha_bg):
    trans_i = prod_{k<i} (1 - a_k), weights = a trans."""
    return scan_graph(up(alpha_all, dtype))


def alpha_weights_backward(sdf, n, raydir, t, gain, car, mask, alpha_bg, alpha_fg_used, g_alpha, g_trans, g_weights):
    """Gradients of (alpha_fg, trans, weights) by autograd.  The scan is evaluated at `alpha_fg_used` (the kernel's fp32 alpha:
    a + (used - a).detach(), so the value is the kernel's and the derivative the formula's) -- otherwise 1 / (1 - a) would turn
    alpha's rounding into a wide bound on everything behind an almost opaque sample.  An absent upstream gradient is zero.
    -> dict: g_sdf (R,N), g_n (R,N,3), g_gain_ray (R,), g_alpha_bg (R,Nb) with, per element, `mag` = sum of |terms| and the
    pieces the bound needs: `horner` (N+Nb,) = roundings of the scan ahead of and behind sample i, `hmag_*` = horner times the
    share of sum|terms| that came through the scan (what arrives as g_alpha_fg does not pass through it), `sig` = what the two
    sigmoid' factors c (1 - c) add in absolute terms (c is rounded to u near 1 and 1 - c is then exact: an error of u c, not of
    u c (1 - c)), `xs` = |x0| + |x1| + G (1 + rho): what the sigmoids' arguments are off by, over u (`alpha_roundings`)."""
    sdf, n, raydir, t, mask = up(sdf), up(n), up(raydir), up(t), up(mask).reshape(-1)
    R, N = sdf.shape
    abg = up(alpha_bg) if alpha_bg is not None and alpha_bg.numel() else torch.zeros(R, 0, dtype=F64)
    Nb = abg.shape[1]
    S = N + Nb
    sdf_l, n_l, abg_l = sdf.clone().requires_grad_(True), n.clone().requires_grad_(True), abg.clone().requires_grad_(True)
    gain_l = up(gain).reshape(()).expand(R, N).clone().requires_grad_(True)          # one leaf per sample: the terms of g_gain_ray
    car = up(car).reshape(())
    p = alpha_parts(sdf_l, n_l, raydir, t, gain_l, car)
    a = p["alpha"]
    a_used = a + (up(alpha_fg_used) - a).detach()
    a_all = torch.cat([a_used * mask[:, None], abg_l], dim=1)
    trans, weights = scan_graph(a_all)
    outs, gs = [], []
    for o, g in ((a, g_alpha), (trans, g_trans), (weights, g_weights)):
        if g is not None:
            outs.append(o)
            gs.append(up(g).reshape(o.shape))
    z = lambda l: torch.zeros_like(l)
    if outs:
        got = torch.autograd.grad(outs, [sdf_l, n_l, gain_l, abg_l], gs, allow_unused=True)
        g_sdf, g_n, g_gain, g_bg = [z(l) if g is None else g for g, l in zip(got, (sdf_l, n_l, gain_l, abg_l))]
    else:
        g_sdf, g_n, g_gain, g_bg = z(sdf_l), z(n_l), z(gain_l), z(abg_l)
    # magnitudes, by the recurrence of the scan with absolute values
    A, X, T = a_all.detach(), 1.0 - a_all.detach(), trans.detach()
    gT = up(g_trans).reshape(R, S).abs() if g_trans is not None else torch.zeros(R, S, dtype=F64)
    gw = up(g_weights).reshape(R, S).abs() if g_weights is not None else torch.zeros(R, S, dtype=F64)
    H = gT + gw * A
    Sabs = torch.zeros(R, S, dtype=F64)
    s = torch.zeros(R, dtype=F64)
    for j in range(S - 1, -1, -1):
        Sabs[:, j] = s
        s = H[:, j] + X[:, j] * s
    magA = gw * T + T * Sabs
    idx = torch.arange(S, dtype=F64)
    horner = (3.0 * idx + 2.0) + 2.0 * (S - 1 - idx)            # trans_i as the kernel read it; two roundings per step behind i
    pd = {k: v.detach() for k, v in p.items()}
    passes = ((pd["q"] >= 0) & (pd["q"] <= 1)).to(F64)
    gq_scan = magA[:, :N] * mask.abs()[:, None] * passes              # the share that came through the scan: K_i applies to it alone
    gq = gq_scan + (up(g_alpha).reshape(R, N).abs() * passes if g_alpha is not None else 0.0)
    hq = horner[None, :N] * gq_scan
    v = pd["c0"] + E5
    p0, p1 = pd["c1"] / (v * v), 1.0 / v
    d0, d1 = pd["c0"] * (1 - pd["c0"]), pd["c1"] * (1 - pd["c1"])
    g = up(gain).reshape(())
    lin = p0 * d0 + p1 * d1
    sig = p0 * pd["c0"] + p1 * pd["c1"]
    dic = 0.5 * (1.0 - car) * (pd["a0"] > 0) + car * (pd["a1"] > 0)
    to_n = g * pd["delta"].abs() * 0.5 * dic
    _, rho, G = alpha_roundings(pd, g, car)
    return dict(g_sdf=g_sdf, g_n=g_n, g_gain_ray=g_gain.sum(1), g_alpha_bg=g_bg,
                mag_sdf=gq * lin * g, sig_sdf=gq * sig * g,
                mag_n=(gq * lin * to_n)[..., None] * raydir.abs()[:, None, :], sig_n=(gq * sig * to_n)[..., None] * raydir.abs()[:, None, :],
                mag_gain=gq * (p0 * d0 * pd["s0"].abs() + p1 * d1 * pd["s1"].abs()),
                sig_gain=gq * (p0 * pd["c0"] * pd["s0"].abs() + p1 * pd["c1"] * pd["s1"].abs()),
                hmag_sdf=hq * lin * g, hmag_n=(hq * lin * to_n)[..., None] * raydir.abs()[:, None, :],
                hmag_gain=hq * (p0 * d0 * pd["s0"].abs() + p1 * d1 * pd["s1"].abs()),
                mag_bg=magA[:, N:], horner=horner, xs=pd["x0"].abs() + pd["x1"].abs() + G * (1 + rho), T_gain=N)


def scan_graph(a_all):
    one_m = 1.0 - a_all
    trans = torch.cat([torch.ones_like(a_all[:, :1]), torch.cumprod(one_m, dim=1)[:, :-1]], dim=1)
    return trans, a_all * trans


def alpha_kink_distance(sdf, n, raydir, t, gain, car):
    """Smallest distance of a sample's kink arguments -- the two relus of iter_cos, clamp(q, 0, 1) -- from their kinks, over
    the margin KINK max(1, |operands|): >= 1 everywhere means that no sample is inside the margin.  (R,N)."""
    p = alpha_parts(up(sdf), up(n), up(raydir), up(t), up(gain).reshape(()), up(car).reshape(()))
    ops = (up(raydir)[:, None, :] * up(n)).abs().sum(-1).clamp(min=1.0)
    dist = torch.minimum(p["a0"].abs() / ops, p["a1"].abs() / ops)
    dist = torch.minimum(dist, torch.minimum(p["q"].abs(), (p["q"] - 1.0).abs()))
    return dist / KINK


def build_alpha(R, N, Nb, seed, mask_values=(0.0, 0.25, 1.0), opaque=True, bg_one=True, unsorted=True):
    """fp32 CPU inputs in the kernel's layout.  |gain sdf| <= 16 (gain 40, |sdf| <= 0.4; the planted opaque sample apart).
    Planted, where the shape has room: ray 0 opaque at sample 3 (gain s = -1000: both sigmoids are 0 in fp32 and in fp64, q is
    1e-5 / 1e-5 = 1 exactly), one background alpha of 1, three samples of ray R-1 with t unsorted (q < 0).
    -> dict of tensors + `exact` (R,N) bool: the planted exact-kink samples, which the margin does not apply to."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    gain, car = torch.tensor([40.0]), torch.tensor([0.3])
    raydir = torch.nn.functional.normalize(rn(R, 3), dim=-1)
    t = torch.sort(torch.rand(R, N + 1, generator=g) * 3.0, dim=1).values
    sdf = (rn(R, N) * 0.05).clamp(-0.4, 0.4)
    sdf[:, ::5] = (torch.rand(R, N, generator=g) * 0.2 + 0.2)[:, ::5]                  # far outside: gain sdf in [8, 16]
    n = rn(R, N, 3)
    exact = torch.zeros(R, N, dtype=torch.bool)
    if unsorted and N >= 8:
        k = min(N - 3, 5)
        t[R - 1, k + 1] = t[R - 1, k] - 0.5                                               # delta < 0 at k, a large delta > 0 at k + 1
        sdf[R - 1, k] = 0.01
        n[R - 1, k] = -2.0 * raydir[R - 1]                                                # tc = -2: both relus open, ic = -(1.05 + 0.6)
    if opaque and N >= 5:
        sdf[0, 3] = -25.0
        exact[0, 3] = True
    for _ in range(200):
        bad = (alpha_kink_distance(sdf, n, raydir, t, gain, car) < 1.0) & ~exact
        if not bool(bad.any()):
            break
        n[bad] = rn(int(bad.sum()), 3)
        sdf[bad] = (rn(int(bad.sum())) * 0.05).clamp(-0.4, 0.4)
    else:
        raise AssertionError("build_alpha: a kink inside the margin after 200 redraws")
    mask = torch.tensor(mask_values)[torch.randint(0, len(mask_values), (R,), generator=g)]
    mask[0] = 1.0
    abg = torch.rand(R, Nb, generator=g) * 0.2
    if bg_one and Nb:
        abg[R - 1, 0] = 1.0
    return dict(sdf=sdf, n=n, raydir=raydir, t=t, gain=gain, car=car, mask=mask, alpha_bg=abg, exact=exact)


# ---- (b), (c) the VR integrals (python/renderer.py:84-87) -----------------------------------------------------------------------
def integrate(w, x, dtype=F64):
    """w (R,S), x (R,S,C) -> (out (R,C), sum|terms|, T = S)."""
    terms = up(w, dtype)[:, :, None] * up(x, dtype)
    return terms.sum(1), terms.abs().sum(1), x.shape[1]


def integrate_backward(w, x, g, dtype=F64):
    """-> (gx (R,S,C) = w g, one product; gw (R,S) = sum_c x g, its sum|terms|, T = C)."""
    w, x, g = up(w, dtype), up(x, dtype), up(g, dtype)
    terms = x * g[:, None, :]
    return w[:, :, None] * g[:, None, :], terms.sum(-1), terms.abs().sum(-1), x.shape[2]


def integrate_many_backward(w, xs, offs, gs, dtype=F64):
    """Segments x_k (R,S_k,C_k) against w[:, off_k : off_k + S_k]; g_k (R,C_k) or None.
    -> (list of gx_k or None, gw (R,S_all), its sum|terms|, T (S_all,) = channels of the segments that cover j with a gradient)."""
    w = up(w, dtype)
    R, S_all = w.shape
    gw, mag, T, gxs = torch.zeros(R, S_all, dtype=dtype), torch.zeros(R, S_all, dtype=dtype), torch.zeros(S_all, dtype=dtype), []
    for x, off, g in zip(xs, offs, gs):
        if g is None:
            gxs.append(None)
            continue
        S = x.shape[1]
        gx, v, m, C = integrate_backward(w[:, off:off + S], x, g, dtype)
        gxs.append(gx)
        gw[:, off:off + S] += v
        mag[:, off:off + S] += m
        T[off:off + S] += C
    return gxs, gw, mag, T


# launch geometry, copied from the host code as integer arithmetic
def rd_pow2(C):
    t = 1
    while t < C and t < 256:
        t <<= 1
    return t


def integrate_geometry(C):
    """k_integrate: (TX, TY, number of c0 trips)."""
    TX = rd_pow2(C)
    return TX, 256 // TX, (C + TX - 1) // TX


def integrate_bwd_geometry(S, C):
    """k_integrate_bwd: ('thread' | 'wave' per sample, lane trips over the channels, sample trips of a workgroup)."""
    if C <= 4:
        return "thread", 1, (S + 255) // 256
    return "wave", (C + 63) // 64, (S + 3) // 4


def integrate_many_geometry(Cs):
    """k_integrate_many: ny and, per segment, (TX, TY, [(blockIdx.y, trip, c0) for every chunk that holds a channel])."""
    ny = min(8, (max(max(Cs), 1) + 63) // 64)
    segs = []
    for C in Cs:
        TX = min(rd_pow2(C), 64)
        chunks = []
        for y in range(ny):
            c0, trip = y * TX, 0
            while c0 < C:
                chunks.append((y, trip, c0))
                c0 += ny * TX
                trip += 1
        segs.append((TX, 256 // TX, chunks))
    return ny, segs


def integrate_many_bwd_geometry(R, S_all):
    """k_integrate_many_bwd: ny and the owner [(blockIdx.y, wave, trip)] of every weight position j, in the order of the walk."""
    ny = max(1, min((4096 + R - 1) // R, (S_all + 3) // 4))
    owners = {}
    for y in range(ny):
        for wave in range(4):
            j, trip = y * 4 + wave, 0
            while j < S_all:
                owners.setdefault(j, []).append((y, wave, trip))
                j += ny * 4
                trip += 1
    return ny, owners


def vec_trips(C):
    """Lane trips of a segment in k_integrate_many_bwd: ('v4' | 'scalar', trips)."""
    return ("v4", (C + 255) // 256) if C % 4 == 0 else ("scalar", (C + 63) // 64)


# ---- (d) light integrals (python/renderer.py:105-161, python/specular_brdf.py:23-199) ----------------------------------------------
def _expand(t, M):
    """(R,k) -> a leaf (R,M,k): the gradient of a per-ray input, one light at a time."""
    return t[:, None, :].expand(t.shape[0], M, t.shape[1]).clone().requires_grad_(True)


def _dot(a, b):
    return (a * b).sum(-1)


def _backward_terms(out, leaves, g):
    """Backpropagate g (R,K) one column at a time.  -> per leaf (sum over the columns, sum of the absolute values)."""
    vals, mags = [torch.zeros_like(l) for l in leaves], [torch.zeros_like(l) for l in leaves]
    for k in range(g.shape[1]):
        gk = torch.zeros_like(g)
        gk[:, k] = g[:, k]
        got = torch.autograd.grad(out, leaves, gk, retain_graph=True, allow_unused=True)
        for v, m, t in zip(vals, mags, got):
            if t is not None:
                v += t
                m += t.abs()
    return vals, mags


def diffuse_light(normal, light, soft_vis, env, eps, g=None, dtype=F64):
    """renderer.py:117-118: mean_m(soft_vis env clamp(n.l, eps)).  normal (R,3), light (R,M,3), soft_vis (R,M), env (R,M,C).
    The magnitudes take sum_i |n_i l_i| for n.l: the dot's rounding error scales with it, not with what is left after it cancels.
    -> dict(out, mag, T = M [, g_normal, mag_normal, g_soft_vis, mag_soft_vis, g_env, mag_env])."""
    n, l, sv, e = up(normal, dtype), up(light, dtype), up(soft_vis, dtype), up(env, dtype)
    R, M, C = e.shape
    eps = f32(eps)
    n_l = n.clone().requires_grad_(True)
    sv_l, e_l = sv.clone().requires_grad_(True), e.clone().requires_grad_(True)
    raw = _dot(n_l[:, None, :], l)
    c = raw.clamp(min=eps)
    adot = (n[:, None, :] * l).abs().sum(-1).clamp(min=eps)
    terms = sv_l[..., None] * e_l * c[..., None] / M
    out = terms.sum(1)
    res = dict(out=out.detach(), mag=(sv[..., None] * e * adot[..., None]).abs().sum(1) / M, T=M)
    if g is not None:
        g = up(g, dtype)
        gn, gsv, ge = torch.autograd.grad(out, [n_l, sv_l, e_l], g)
        ge_mag = (g.abs()[:, None, :] * e.abs()).sum(-1) / M
        passes = (raw.detach() >= eps).to(dtype)
        res.update(g_normal=gn, mag_normal=((ge_mag * sv.abs() * passes)[..., None] * l.abs()).sum(1), g_soft_vis=gsv,
                   mag_soft_vis=ge_mag * adot, g_env=ge, mag_env=g.abs()[:, None, :] / M * (sv.abs() * adot)[..., None])
    return res


def spec_S(nol, nov, noh, voh, r, model, sampling):
    """specular_brdf.py:40-118 (filament, model 0) / :121-191 (ue4, 1) without Fresnel and mask: (W K, f) with
    Fs = sc + (1 - sc) f.  sampling 0 importance, 1 uniform."""
    eps = 1e-6
    if model == 0:
        a2 = r ** 2
        V1 = lambda u_: 1 / (u_ + (a2 + (1 - a2) * u_ ** 2) ** 0.5 + eps)
        W = V1(nol) * V1(nov)
        f = (1 - voh) ** 5
        if sampling == 0:
            K = 4 * voh / noh
        else:
            K = math.pi * (a2 / (math.pi * (noh ** 2 * (a2 - 1) + 1) ** 2 + eps))
    else:
        a2 = (r ** 2) ** 2
        k = (r + 1) ** 2 / 8
        G1 = lambda u_: u_ / (u_ * (1 - k) + k + eps)
        W = G1(nol) * G1(nov)
        f = 2 ** ((-5.55473 * voh - 6.98316) * voh)
        if sampling == 0:
            K = voh / (noh * nov)
        else:
            K = math.pi * (a2 / (math.pi * (noh ** 2 * (a2 - 1) + 1) ** 2 + eps)) / (4 * nov * nol)
    return W * K, f


def _spec_terms(n_e, v, l, r_e, sc_e, eps, model, sampling):
    """Per light: (sBRDF (R,M,3) with the mask, clamped n.l (R,M)).  n_e (R,M,3), v (R,3), r_e (R,M), sc_e (R,M,3)."""
    v_e = v[:, None, :].expand_as(l)
    h = l + v_e
    h = (h / torch.sqrt((h * h).sum(-1, keepdim=True))).detach()
    rnol, rnov, rnoh, rvoh = _dot(n_e, l), _dot(n_e, v_e), _dot(n_e, h), _dot(v_e, h)
    mask = ((rnol > eps) & (rnov > eps) & (rnoh > eps)).to(l.dtype).detach()
    nol, nov, noh, voh = (x.clamp(min=eps) for x in (rnol, rnov, rnoh, rvoh))
    WK, f = spec_S(nol, nov, noh, voh, r_e, model, sampling)
    Fs = sc_e + (1 - sc_e) * f[..., None]
    return (WK * mask)[..., None] * Fs, nol


def specular_light(normal, view, light, rough, spec, soft_vis, env, eps, weight, model=0, sampling=0, split=False, g=None, dtype=F64):
    """renderer.py:136-161.  normal, view (R,3), light (R,M,3), rough (R,), spec (R,3), soft_vis (R,M), env (R,M,C), C 1 | 3.
    out = weight mean_m(sBRDF soft_vis env n.l), or with the split sum weight mean_m(soft_vis env) mean_m(sBRDF n.l).
    -> dict(out (R,3), mag, T [, g_normal (R,3), g_rough (R,), g_spec (R,3) with mag_* over the T = 3 M terms (light x colour
    channel), g_soft_vis (R,M), g_env (R,M,C) with mag_* over their 3 | 3 / C colour-channel terms])."""
    n, v, l, sv, e = (up(x, dtype) for x in (normal, view, light, soft_vis, env))
    R, M, C = e.shape
    eps, weight = f32(eps), f32(weight)
    n_e = _expand(n, M)
    r_e = _expand(up(rough, dtype).reshape(R, 1), M)
    sc_e = _expand(up(spec, dtype), M)
    sv_l, e_l = sv.clone().requires_grad_(True), e.clone().requires_grad_(True)
    sB, nol = _spec_terms(n_e, v, l, r_e[..., 0], sc_e, eps, model, sampling)
    e3 = e_l.expand(R, M, 3)
    if split:
        A, B = sv_l[..., None] * e3, sB * nol[..., None]
        out = weight * A.mean(1) * B.mean(1)
        mag, T = weight * A.abs().mean(1) * B.abs().mean(1), 2 * M
    else:
        terms = weight * sB * sv_l[..., None] * e3 * nol[..., None] / M
        out, mag, T = terms.sum(1), terms.abs().sum(1), M
    res = dict(out=out.detach(), mag=mag.detach(), T=T)
    if g is not None:
        (gn, gr, gs, gsv, ge), (mn, mr, ms, msv, me) = _backward_terms(out, [n_e, r_e, sc_e, sv_l, e_l], up(g, dtype))
        res.update(g_normal=gn.sum(1), mag_normal=mn.sum(1), g_rough=gr.sum(1)[:, 0], mag_rough=mr.sum(1)[:, 0], g_spec=gs.sum(1),
                   mag_spec=ms.sum(1), g_soft_vis=gsv, mag_soft_vis=msv, g_env=ge, mag_env=me, T_ray=3 * M)
    return res


def light_act(kind, beta, v):
    """python/network.py:288-296, 372-376 `act_last`: 0 identity, 1 softplus(beta) with torch's threshold 20, 2 sigmoid, 3 relu."""
    if kind == 1:
        return torch.nn.functional.softplus(v, beta=beta, threshold=20.0)
    if kind == 2:
        return torch.sigmoid(v)
    if kind == 3:
        return torch.relu(v)
    return v


def direct_light(normal, view, dirs, raw_sv, raw_env, pix, bg, acts, params, entangle, g=None, dtype=F64):
    """renderer.py:105-178, default branch.  dirs (R,2M,3) [diffuse | specular], raw_sv (R,2M), raw_env (R,2M,C), pix (R,9),
    bg (R,3) | None; acts (sv, env), params (beta_sv, beta_env, ub_env, eps_dot, weight).
    -> dict(color, env_pix, spec_pix with mag_* [, g_normal, g_raw_sv, g_raw_env, g_pix, g_bg with mag_*]); T = M."""
    n, v, dr, rsv, renv, px = (up(x, dtype) for x in (normal, view, dirs, raw_sv, raw_env, pix))
    R, M2, C = renv.shape
    M = M2 // 2
    b_sv, b_env, ub, eps, weight = (f32(p) for p in params)
    n_e = _expand(n, M2)
    rsv_l, renv_l = rsv.clone().requires_grad_(True), renv.clone().requires_grad_(True)
    ro_e, sc_e = _expand(px[:, 1:2], M), _expand(px[:, 2:5], M)
    px_l = px.clone().requires_grad_(True)
    bg_l = up(bg, dtype).clone().requires_grad_(True) if bg is not None else None
    sv = light_act(acts[0], b_sv, rsv_l)
    env = light_act(acts[1], b_env, renv_l)
    if ub > 0:
        env = env.clamp(0.0, ub)
    cs = _dot(n_e[:, :M], dr[:, :M]).clamp(min=eps)
    dterms = sv[:, :M, None] * env[:, :M] * cs[..., None] / M
    env_pix = dterms.sum(1)
    sB, nol = _spec_terms(n_e[:, M:], v, dr[:, M:], ro_e[..., 0], sc_e, eps, 0, 0)
    sterms = weight * sB * sv[:, M:, None] * env[:, M:].expand(R, M, 3) * nol[..., None] / M
    spec_pix = sterms.sum(1)
    imp, photo, base = px_l[:, 0:1], px_l[:, 5:6], px_l[:, 6:9]
    diff = env_pix + imp
    fg = base * diff + photo * spec_pix if entangle else photo * (base * diff + spec_pix)
    color = fg + bg_l if bg_l is not None else fg
    adot = (n[:, None, :] * dr[:, :M]).abs().sum(-1).clamp(min=eps)
    mag_env = (sv[:, :M, None] * env[:, :M] * adot[..., None]).detach().abs().sum(1) / M
    mag_spec = sterms.detach().abs().sum(1)
    ab = px.abs()
    dm = mag_env + ab[:, 0:1]
    mag_color = (ab[:, 6:9] * dm + ab[:, 5:6] * mag_spec) if entangle else ab[:, 5:6] * (ab[:, 6:9] * dm + mag_spec)
    if bg is not None:
        mag_color = mag_color + up(bg, dtype).abs()
    res = dict(color=color.detach(), env_pix=env_pix.detach(), spec_pix=spec_pix.detach(), mag_color=mag_color, mag_env_pix=mag_env,
               mag_spec_pix=mag_spec, T=M)
    if g is not None:
        leaves = [n_e, rsv_l, renv_l, px_l, ro_e, sc_e] + ([bg_l] if bg_l is not None else [])
        vals, mags = _backward_terms(color, leaves, up(g, dtype))
        g_pix, m_pix = vals[3].clone(), mags[3].clone()
        g_pix[:, 1], m_pix[:, 1] = vals[4].sum(1)[:, 0], mags[4].sum(1)[:, 0]
        g_pix[:, 2:5], m_pix[:, 2:5] = vals[5].sum(1), mags[5].sum(1)
        res.update(g_normal=vals[0].sum(1), mag_normal=mags[0].sum(1), g_raw_sv=vals[1], mag_raw_sv=mags[1], g_raw_env=vals[2],
                   mag_raw_env=mags[2], g_pix=g_pix, mag_pix=m_pix, g_bg=vals[6] if bg_l is not None else None, T_ray=3 * M2)
    return res


def light_kink_distance(normal, view, light, eps):
    """Distance of the four clamped dots of every light from eps_dot, over the margin.  (R,M)."""
    n, v, l = up(normal), up(view), up(light)
    v_e = v[:, None, :].expand_as(l)
    h = l + v_e
    h = h / torch.sqrt((h * h).sum(-1, keepdim=True))
    n_e = n[:, None, :].expand_as(l)
    dist = None
    for a, b in ((n_e, l), (n_e, v_e), (n_e, h), (v_e, h)):
        dd = (_dot(a, b) - f32(eps)).abs() / (a * b).abs().sum(-1).clamp(min=1.0)
        dist = dd if dist is None else torch.minimum(dist, dd)
    return dist / KINK


def _draw_lights(normal, view, M, g, eps, below):
    """M unit directions around the normal, `below` of them mirrored under the surface, none with a dot inside the margin."""
    R = normal.shape[0]
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    n_e = normal[:, None, :].expand(R, M, 3)
    under = torch.zeros(R, M, dtype=torch.bool)
    under[:, :min(below, M - 1)] = True
    light = unit(n_e + 0.8 * torch.randn(R, M, 3, generator=g))
    light[under] = -light[under]
    for _ in range(200):
        bad = light_kink_distance(normal, view, light, eps) < 1.0
        if not bool(bad.any()):
            return light
        fresh = unit(n_e + 0.8 * torch.randn(R, M, 3, generator=g))
        fresh[under] = -fresh[under]
        light[bad] = fresh[bad]
    raise AssertionError("_draw_lights: a kink inside the margin after 200 redraws")


def build_lights(R, M, C, seed, eps=1e-8, below=3):
    """Unit normal, view and M light directions around the normal, `below` of them under the surface (the masks); roughness in
    [0.1, 0.9], specular colour, soft visibility, env > 0, upstream gradients.  No dot within the margin of eps_dot."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    normal = unit(rn(R, 3))
    for _ in range(200):
        view = unit(normal + 0.7 * rn(R, 3))
        nov = (normal * view).sum(-1).double()
        if bool(((nov - f32(eps)).abs() >= KINK).all()):
            break
    light = _draw_lights(normal, view, M, g, eps, below)
    return dict(normal=normal, view=view, light=light, rough=torch.rand(R, generator=g) * 0.8 + 0.1, spec=torch.rand(R, 3, generator=g),
                soft_vis=torch.rand(R, M, generator=g), env=torch.rand(R, M, C, generator=g) + 0.1, g=rn(R, 3), gC=rn(R, C), eps=eps)


SOFTPLUS_EDGE = (19.5, 20.0, 20.5)


def act_kink_distance(kind, beta, ub, raw):
    """Distance of a raw net output from the relu's kink and of the activated value from the ub_env clamp (0 and ub), over the
    margin.  softplus' threshold is no kink of the value or the slope beyond 2e-9: it is planted, not avoided."""
    raw = up(raw)
    dist = torch.full_like(raw, float("inf"))
    if kind == 3:
        dist = raw.abs()
    if ub > 0:
        y = light_act(kind, beta, raw)
        dist = torch.minimum(dist, torch.minimum(y.abs(), (y - f32(ub)).abs()) / max(1.0, f32(ub)))
    return dist / KINK


def build_direct(R, M, C, seed, acts, betas, ub, eps=1e-8, with_bg=True):
    """Inputs of direct_light: two sets of lights (diffuse, specular), raw net outputs (softplus: beta v = 19.5, 20, 20.5
    planted), pix with roughness in [0.1, 0.9] and specular in [0, 0.16], background."""
    a = build_lights(R, M, C, seed, eps)
    g = torch.Generator().manual_seed(seed + 7)
    rn = lambda *s: torch.randn(*s, generator=g)
    dirs = torch.cat([a["light"], _draw_lights(a["normal"], a["view"], M, g, eps, 2)], dim=1)
    raw_sv, raw_env = rn(R, 2 * M) * 2.0, rn(R, 2 * M, C) * 1.5
    for raw, kind, beta, u_ in ((raw_sv, acts[0], betas[0], -1.0), (raw_env, acts[1], betas[1], ub)):
        for _ in range(200):
            bad = act_kink_distance(kind, beta, u_, raw) < 1.0
            if not bool(bad.any()):
                break
            raw[bad] = rn(int(bad.sum())) * 1.5
        else:
            raise AssertionError("build_direct: an activation kink inside the margin after 200 redraws")
        if kind == 1 and u_ <= 0:
            flat = raw.view(-1)
            for i, e_ in enumerate(SOFTPLUS_EDGE[:flat.numel()]):
                flat[i] = e_ / beta
    pix = torch.rand(R, 9, generator=g)
    pix[:, 1] = pix[:, 1] * 0.8 + 0.1
    pix[:, 2:5] *= 0.16
    return dict(normal=a["normal"], view=a["view"], dirs=dirs, raw_sv=raw_sv, raw_env=raw_env, pix=pix,
                bg=torch.rand(R, 3, generator=g) if with_bg else None, g=rn(R, 3))


# ---- (e) material head (python/network.py:262, 335, 423, 456-463, 498-508; python/loss.py:117-166), gain (network.py:229-231) ----
def _softplus(x):
    return torch.nn.functional.softplus(x, beta=1.0, threshold=20.0)


def material_parts(raw_bc, raw_ptb, raw_imp, raw_photo, pg, raw_rough, raw_spec, cfg):
    """Tensors of one dtype, (R,N,k).  cfg = (remap, entangle, sym, rough_lb, spec_scale, prior_r, prior_s).
    -> (V (R,N,9), aux (R,N,10), prior terms: list of five (R,N*) tensors whose row sums are the priors, kink arguments)."""
    remap, entangle, sym, lb, scale, pr, ps = cfg
    R, N = raw_bc.shape[:2]
    bc, pt = torch.sigmoid(raw_bc), torch.sigmoid(raw_ptb)
    imp, photo = torch.sigmoid(raw_imp), torch.sigmoid(pg * raw_photo)
    r0 = torch.sigmoid(raw_rough[..., 0:1])
    r1 = r0 ** 2 if remap else r0
    ro = r1.clamp(lb, 1.0)
    sr = _softplus(raw_rough[..., 1:2])
    s0 = torch.sigmoid(raw_spec[..., :3])
    sp = 0.16 * s0 ** 2 if remap else scale * s0
    ss = _softplus(raw_spec[..., 3:])
    V = torch.cat([imp, ro, sp, photo, bc * photo if entangle else bc], dim=-1)
    aux = torch.cat([bc, pt, sr, ss], dim=-1)
    bcp = bc if sym else bc.detach()
    lsr, lss = torch.log(sr), torch.log(ss)
    terms = [(bcp - pt).abs().reshape(R, -1), ((ro - pr).abs() / sr).reshape(R, -1), lsr.clamp(1e-5, 1e5).reshape(R, -1),
             ((sp - ps).abs() / ss).reshape(R, -1), lss.clamp(1e-5, 1e5).reshape(R, -1)]
    # what a term's rounding error scales with: a difference by the sum of its operands, a logarithm by 1 + |log|
    tmags = [(bc + pt).reshape(R, -1), ((ro + pr) / sr).reshape(R, -1), (lsr.abs() + 1.0).reshape(R, -1),
             ((sp + ps) / ss).reshape(R, -1), (lss.abs() + 1.0).reshape(R, -1)]
    kinks = dict(bc_pt=bc - pt, rough_lb=r1 - lb, ro_prior=ro - pr, sp_prior=sp - ps, log_sr=lsr - 1e-5, log_ss=lss - 1e-5)
    parts = dict(ro=ro, sr=sr, sp=sp, ss=ss, tmags=tmags, h_r=raw_rough[..., 1:2], h_s=raw_spec[..., 3:])
    return V, aux, terms, kinks, parts


def material_head(raws, pg, cfg, gV=None, g_prior=None, dtype=F64):
    """raws = (raw_bc (R,N,3), raw_ptb (R,N,3), raw_imp (R,N,1), raw_photo (R,N,1), raw_rough (R,N,2), raw_spec (R,N,6)).
    -> dict(V, aux, prior (R,5), mag_prior, T_prior (5,) [, grads: six tensors, mags: their sum|terms| over the 14 upstream
    components, extra: the absolute part of the std columns' error scale])."""
    cfg = tuple(cfg[:3]) + tuple(f32(c) for c in cfg[3:])
    leaves = [up(t, dtype).clone().requires_grad_(True) for t in raws]
    pgv = up(pg, dtype).reshape(())
    V, aux, terms, _, parts = material_parts(leaves[0], leaves[1], leaves[2], leaves[3], pgv, leaves[4], leaves[5], cfg)
    prior = torch.stack([t.sum(1) for t in terms], dim=-1)
    res = dict(V=V.detach(), aux=aux.detach(), prior=prior.detach(), mag_prior=torch.stack([t.detach().abs().sum(1) for t in parts["tmags"]], dim=-1),
               T_prior=torch.tensor([t.shape[1] for t in terms], dtype=dtype))
    if gV is not None:
        R, N = V.shape[:2]
        vals, mags = [torch.zeros_like(l) for l in leaves], [torch.zeros_like(l) for l in leaves]
        gVd = up(gV, dtype).reshape(R, N, 9)
        ups = []
        for k in range(9):
            gk = torch.zeros_like(gVd)
            gk[..., k] = gVd[..., k]
            ups.append((V, gk))
        if g_prior is not None:
            gp = up(g_prior, dtype)
            for k in range(5):
                gk = torch.zeros_like(gp)
                gk[:, k] = gp[:, k]
                ups.append((prior, gk))
        for o, gk in ups:
            got = torch.autograd.grad(o, leaves, gk, retain_graph=True, allow_unused=True)
            for v, m, t in zip(vals, mags, got):
                if t is not None:
                    v += t
                    m += t.abs()
        # the std gradients hold |ro - prior| / std^2: the difference's rounding scales with ro + prior
        pd = {k: v.detach() for k, v in parts.items() if k != "tmags"}
        extra = [torch.zeros_like(l) for l in leaves]
        if g_prior is not None:
            gp = up(g_prior, dtype).abs()
            extra[4][..., 1:2] = gp[:, None, 1:2] * (pd["ro"] + cfg[5]) / pd["sr"] ** 2 * torch.sigmoid(pd["h_r"])
            extra[5][..., 3:] = gp[:, None, 3:4] * (pd["sp"] + cfg[6]) / pd["ss"] ** 2 * torch.sigmoid(pd["h_s"])
        res.update(grads=vals, mags=mags, extra=extra)
    return res


def material_kink_distance(raws, pg, cfg):
    """Per sample: the smallest distance of a kink argument -- sign(bc - pt), the roughness bounds, sign(ro - prior_r),
    sign(sp - prior_s), clamp(log std, 1e-5, 1e5) -- from its kink, over the margin.  (R,N)."""
    cfg = tuple(cfg[:3]) + tuple(f32(c) for c in cfg[3:])
    _, _, _, k, _ = material_parts(*[up(t) for t in raws[:4]], up(pg).reshape(()), up(raws[4]), up(raws[5]), cfg)
    dist = None
    for name, v in k.items():
        ops = (v + 1e-5).abs().clamp(min=1.0) if name.startswith("log") else 1.0          # |log std| can reach 1e2; 1e5 is out of reach
        dd = (v.abs() / ops).amin(-1)
        dist = dd if dist is None else torch.minimum(dist, dd)
    return dist / KINK


STD_EDGE = (19.5, 20.0, 20.5, -30.0, -40.0)


def build_material(R, N, seed, cfg):
    """Raw net outputs randn x 1.5; then the raw std inputs of the first samples (roughness) and of the last ones (specular) at
    softplus' threshold (19.5, 20, 20.5) and at large negative values (-30, -40: 1 / std^2 still finite in fp32).
    -> (raws, photo gain, gV, g_prior)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g) * 1.5
    raws = [rn(R, N, 3), rn(R, N, 3), rn(R, N, 1), rn(R, N, 1), rn(R, N, 2), rn(R, N, 6)]
    pg = torch.tensor([1.3])
    for _ in range(200):
        bad = material_kink_distance(raws, pg, cfg) < 1.0
        if not bool(bad.any()):
            break
        k = int(bad.sum())
        for i, w in ((0, 3), (1, 3), (4, 2), (5, 6)):
            raws[i][bad] = rn(k, w)
    else:
        raise AssertionError("build_material: a kink inside the margin after 200 redraws")
    flat_r, flat_s = raws[4].view(-1, 2), raws[5].view(-1, 6)
    for i, e_ in enumerate(STD_EDGE[:flat_r.shape[0]]):
        flat_r[i, 1] = e_
        flat_s[-1 - i, 3 + i % 3] = e_
    assert bool((material_kink_distance(raws, pg, cfg) >= 1.0).all())
    return raws, pg, rn(R, N, 9) / 1.5, rn(R, 5) / 1.5


def gain(p, scale, lo, hi, g=None, dtype=F64):
    """python/network.py:229-231: clip(exp(scale p), lo, hi).  -> (value, unclamped exp, gradient or None)."""
    p_l = up(p, dtype).clone().requires_grad_(True)
    e = torch.exp(p_l * f32(scale))
    out = e.clamp(f32(lo), f32(hi))
    gp = torch.autograd.grad(out, p_l, up(g, dtype))[0] if g is not None else None
    return out.detach(), e.detach(), gp


# ---- the shapes of tests/test_gpu_rays.py (the CPU tests show which path each one enters) ---------------------------------------
RAYS = (1, 3, 130)
ALPHA_SHAPES = ((1, 0), (63, 1), (64, 0), (65, 0), (200, 56), (480, 32))                      # (N, Nb); 512 slots is the limit
INTEGRATE_SHAPES = ((1, 1), (33, 6), (7, 4), (7, 5), (130, 64), (130, 65), (9, 256), (9, 257), (9, 300), (300, 1))      # (S, C)
MANY_FWD = dict(R=2, S_all=9, widths=(3, 64, 65, 256, 520), lds=(3, 64, 66, 259, 530))
MANY_BWD = (dict(R=2, S_all=9, widths=(3, 64, 65, 256, 520, 260), lds=(3, 64, 66, 259, 530, 261)),      # six segments: the limit
            dict(R=2, S_all=9, widths=(258, 260, 9), lds=(259, 263, 9)))
MANY_ONE_RAY = dict(R=1, S_all=40, widths=(3, 20), lds=(3, 21))
MANY_STRIDE = dict(R=5000, S_all=9, widths=(3, 9), lds=(3, 9))
LIGHT_M = (1, 63, 64, 65, 127, 128, 129, 300)
MATERIAL_N = (1, 127, 128, 129, 300, 1030)


def wave_fill(M, threads=SH_THREADS):
    """A workgroup of `threads` (two waves of 64) over M items, `for (m = threadIdx.x; m < M; m += threads)`:
    (items the first wave handles, items the second wave handles, passes of thread 0)."""
    first = sum(1 for m in range(M) if (m % threads) < 64)
    return first, M - first, (M + threads - 1) // threads
