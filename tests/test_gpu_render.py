"""Volume-rendering kernels (csrc/render.hip) vs the stock-op composite of renderer.py:55-87 under
autograd, in fp64 on the GPU: values and every gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def composite_alpha_weights(sdf, n, raydir, t_fg, gain, car, mask, alpha_bg):
    """renderer.py:55-67, :79-82 written with stock ops (any dtype)."""
    rd = raydir.reshape(raydir.shape[0], raydir.shape[1], 1, 3)
    car = car.reshape(1, 1, 1, 1)
    true_cos = (rd * n).sum(-1, keepdim=True)
    iter_cos = -(torch.relu(-true_cos * 0.5 + 0.5) * (1.0 - car) + torch.relu(-true_cos) * car)
    delta = t_fg[:, :, 1:, :] - t_fg[:, :, :-1, :]
    sdf1 = sdf + iter_cos * delta * 0.5
    sdf0 = sdf - iter_cos * delta * 0.5
    g = gain.reshape(1, 1, 1, 1)
    cdf0, cdf1 = torch.sigmoid(g * sdf0), torch.sigmoid(g * sdf1)
    alpha_fg = ((cdf0 - cdf1 + 1e-5) / (cdf0 + 1e-5)).clamp(0.0, 1.0)
    alpha = torch.cat([alpha_fg * mask, alpha_bg], dim=2)
    one_m = 1 - alpha
    trans = torch.cat([torch.ones_like(one_m[:, :, :1]), torch.cumprod(one_m, dim=2)[:, :, :-1]], dim=2)
    return alpha_fg, trans, alpha * trans


def _inputs(B, R, N, Nb, seed, gpu, opaque=False):
    rng = np.random.RandomState(seed)
    f = lambda *s: torch.tensor(rng.randn(*s), dtype=torch.float64, device=gpu)
    sdf = f(B, R, N, 1) * 0.05
    if opaque:
        sdf[:, :, N // 2:, :] = -1.0      # alpha hits exactly 1 -> zeros in the cumprod
    n = f(B, R, N, 3)
    rd = f(B, R, 3)
    rd = rd / rd.norm(dim=-1, keepdim=True)
    t = torch.sort(torch.tensor(rng.rand(B, R, N + 1, 1), dtype=torch.float64, device=gpu) * 3.0, dim=2).values
    gain = torch.tensor([40.0], dtype=torch.float64, device=gpu)
    car = torch.tensor([0.3], dtype=torch.float64, device=gpu)
    mask = torch.tensor((rng.rand(B, R, 1, 1) > 0.2).astype(np.float64), device=gpu)
    abg = torch.tensor(rng.rand(B, R, Nb, 1) * 0.2, dtype=torch.float64, device=gpu)
    return sdf, n, rd, t, gain, car, mask, abg


@pytest.mark.parametrize("B,R,N,Nb,opaque", [(1, 37, 128, 32, False), (2, 5, 7, 1, False), (1, 16, 200, 56, False),
                                              (1, 64, 128, 32, True)])
def test_alpha_weights_matches_composite(gpu, B, R, N, Nb, opaque):
    from ndjir_amd.volume import alpha_weights
    ins64 = _inputs(B, R, N, Nb, 11 + N, gpu, opaque)
    req = (0, 1, 4, 7)   # sdf, n, gain, alpha_bg
    a64 = [t.clone().requires_grad_(i in req) for i, t in enumerate(ins64)]
    a32 = [t.float().requires_grad_(i in req) for i, t in enumerate(ins64)]
    ref = composite_alpha_weights(*a64)
    out = alpha_weights(*a32)
    stock32 = composite_alpha_weights(*[t.float() for t in ins64])
    for o, r, s32 in zip(out, ref, stock32):
        # alpha is a ratio of small differences of sigmoids: compare with the fp64 composite at the
        # accuracy the fp32 stock-op composite itself reaches
        err = float((o.detach().double() - r.detach()).abs().max())
        err_stock = float((s32.double() - r.detach()).abs().max())
        assert err < max(4.0 * err_stock, 2e-6), (err, err_stock)
    rng = np.random.RandomState(3)
    gs = [torch.tensor(rng.randn(*r.shape), dtype=torch.float64, device=gpu) for r in ref]
    gref = torch.autograd.grad(ref, [a64[i] for i in req], gs)
    gout = torch.autograd.grad(out, [a32[i] for i in req], [g.float() for g in gs])
    a32s = [t.float().requires_grad_(i in req) for i, t in enumerate(ins64)]
    gstock = torch.autograd.grad(composite_alpha_weights(*a32s), [a32s[i] for i in req], [g.float() for g in gs])
    for name, go, gr, gst in zip(("sdf", "n", "gain", "alpha_bg"), gout, gref, gstock):
        scale = max(float(gr.abs().max()), 1e-6)
        err = float((go.double() - gr).abs().max()) / scale
        err_stock = float((gst.double() - gr).abs().max()) / scale
        assert err < max(4.0 * err_stock, 1e-5), (name, err, err_stock)


def test_alpha_far_outside_the_surface_keeps_its_relative_accuracy(gpu):
    """Rays that pass the object at a distance: gain * sdf in [8, 16], so both sigmoids are within 3e-4 of 1 and alpha =
    (c0 - c1 + 1e-5) / (c0 + 1e-5) is 1e-5 ... 3e-4.  Their fp32 difference carries 2^-24 absolute, 1e-4 ... 3e-3 of such an
    alpha; the pixel normal and the pixel roughness of a grazing ray are ratios of sums of these, and the specular term's
    d / d roughness at roughness -> 0 multiplied that error into a 6e-3 distance of the roughness net's gradients from fp64
    (test_step_parity_given_samples[custom-32-*]).  The kernel forms c0 - c1 as sigmoid(x0) sigmoid(-x1) (1 - exp(x1 - x0)).
    Bound 2^-18 relative, per sample: x1 = gain * s1 (|x1| <= 16) carries two fp32 roundings, 2 * 2^-24 * 16 = 1.9e-6
    absolute, which is the relative error of sigmoid(-x1) ~ exp(-x1); expf / expm1f (2 ulp each), the argument of expm1f
    (3 roundings) and the remaining 5 operations add 15 * 2^-24 = 0.9e-6.  Measured: 8.2e-7 (the fp32 composite with the subtraction: 1.2e-2)."""
    from ndjir_amd.volume import alpha_weights
    B, R, N, Nb = 1, 40, 128, 1
    rng = np.random.RandomState(5)
    r32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu)
    sdf = r32(0.2 + 0.2 * rng.rand(B, R, N, 1))
    n, rd = rng.randn(B, R, N, 3), rng.randn(B, R, 3)
    n, rd = r32(n / np.linalg.norm(n, axis=-1, keepdims=True)), r32(rd / np.linalg.norm(rd, axis=-1, keepdims=True))
    t = r32((np.arange(N + 1).reshape(1, 1, N + 1, 1) + 0.5 * rng.rand(B, R, N + 1, 1)) * (3.0 / N))
    gain, car = r32([40.0]), r32([0.3])
    mask, abg = torch.ones(B, R, 1, 1, device=gpu), r32(rng.rand(B, R, Nb, 1) * 0.2)
    ins = (sdf, n, rd, t, gain, car, mask, abg)
    ref = composite_alpha_weights(*[v.double() for v in ins])[0]
    assert 1e-5 <= float(ref.min()) and float(ref.max()) < 1e-3
    out = alpha_weights(*ins)[0]
    rel = float(((out.double() - ref).abs() / ref).max())
    stock = float(((composite_alpha_weights(*ins)[0].double() - ref).abs() / ref).max())
    print(f"alpha far outside: max relative error {rel:.2e} (fp32 composite with the subtraction: {stock:.2e}), bound {2.0 ** -18:.2e}")
    assert rel <= 2.0 ** -18, (rel, stock)


@pytest.mark.parametrize("R,S_all,off,S,C", [(50, 160, 0, 128, 256), (50, 160, 128, 32, 3), (7, 128, 0, 128, 1),
                                             (3, 33, 0, 33, 6), (9, 160, 0, 128, 300)])
def test_integrate_matches_composite(gpu, R, S_all, off, S, C):
    from ndjir_amd.volume import integrate
    rng = np.random.RandomState(R + C)
    w64 = torch.tensor(rng.rand(1, R, S_all, 1), dtype=torch.float64, device=gpu, requires_grad=True)
    x64 = torch.tensor(rng.randn(1, R, S, C), dtype=torch.float64, device=gpu, requires_grad=True)
    w32 = w64.detach().float().requires_grad_(True)
    x32 = x64.detach().float().requires_grad_(True)
    ref = (w64[:, :, off:off + S, :] * x64).sum(dim=2)
    out = integrate(w32, x32, off)
    assert float((out.double() - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))
    g = torch.tensor(rng.randn(1, R, C), dtype=torch.float64, device=gpu)
    gw64, gx64 = torch.autograd.grad(ref, [w64, x64], g)
    gw32, gx32 = torch.autograd.grad(out, [w32, x32], g.float())
    assert float((gx32.double() - gx64).abs().max()) < 1e-5 * max(1.0, float(gx64.abs().max()))
    assert float((gw32.double() - gw64).abs().max()) < 1e-5 * max(1.0, float(gw64.abs().max()))


@pytest.mark.parametrize("R,N,Nb", [(37, 128, 32), (5, 256, 32), (16, 64, 1)])
def test_integrate_many_matches_composite(gpu, R, N, Nb):
    """volume.integrate_many: the ray's VR integrals (3-, 3-, 20-, 9-wide over the foreground, a column slice of a wider
    array among them, 3-wide over the background) in one launch each way; one of the outputs unused."""
    from ndjir_amd.volume import integrate_many
    rng = np.random.RandomState(R + N)
    w64 = torch.tensor(rng.rand(1, R, N + Nb, 1), dtype=torch.float64, device=gpu, requires_grad=True)
    wide = torch.tensor(rng.randn(1, R, N, 28), dtype=torch.float64, device=gpu, requires_grad=True)
    xs64 = [torch.tensor(rng.randn(1, R, S, C), dtype=torch.float64, device=gpu, requires_grad=True)
            for S, C in ((N, 3), (N, 3), (N, 9), (Nb, 3))]
    offs = [0, 0, 0, 0, N]
    ins64 = xs64[:2] + [wide[..., 3:23]] + xs64[2:]
    ref = [(w64[:, :, o:o + x.shape[2], :] * x).sum(dim=2) for x, o in zip(ins64, offs)]
    w32 = w64.detach().float().requires_grad_(True)
    wide32 = wide.detach().float().requires_grad_(True)
    xs32 = [x.detach().float().requires_grad_(True) for x in xs64]
    out = integrate_many(w32, xs32[:2] + [wide32[..., 3:23]] + xs32[2:], offs)
    for a, b in zip(out, ref):
        assert float((a.double() - b).abs().max()) < 1e-4 * max(1.0, float(b.abs().max()))
    gs = [torch.tensor(rng.randn(*r.shape), dtype=torch.float64, device=gpu) for r in ref]
    use = [0, 2, 3, 4]                                    # the second integral's result is not used
    g64 = torch.autograd.grad([ref[k] for k in use], [w64, wide] + xs64, [gs[k] for k in use], allow_unused=True)
    g32 = torch.autograd.grad([out[k] for k in use], [w32, wide32] + xs32, [gs[k].float() for k in use], allow_unused=True)
    for i, (a, b) in enumerate(zip(g32, g64)):
        if b is None:
            assert a is None, i
            continue
        assert float((a.double() - b).abs().max()) < 1e-5 * max(1.0, float(b.abs().max())), i


def _light_inputs(B, R, M, C, seed, gpu):
    rng = np.random.RandomState(seed)
    f = lambda *s: torch.tensor(rng.randn(*s), dtype=torch.float64, device=gpu)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    normal = unit(f(B, R, 3))
    view = unit(f(B, R, 3) + 1.5 * normal)          # mostly in the upper hemisphere, some grazing / below
    light = unit(f(B, R, M, 3) + 1.0 * normal[:, :, None, :])
    rough = torch.tensor(rng.rand(B, R, 1) * 0.9 + 0.05, dtype=torch.float64, device=gpu)
    spec = torch.tensor(rng.rand(B, R, 3) * 0.16, dtype=torch.float64, device=gpu)
    sv = torch.tensor(rng.rand(B, R, M, 1), dtype=torch.float64, device=gpu)
    env = torch.tensor(rng.rand(B, R, M, C) * 2.0, dtype=torch.float64, device=gpu)
    return normal, view, light, rough, spec, sv, env


@pytest.mark.parametrize("B,R,M,C", [(1, 40, 128, 1), (2, 7, 32, 3), (1, 3, 200, 1)])
def test_diffuse_light_matches_composite(gpu, B, R, M, C):
    from ndjir_amd.specular_brdf import dot
    from ndjir_amd.volume import diffuse_light
    normal, _, light, _, _, sv, env = _light_inputs(B, R, M, C, 5 + M, gpu)
    eps = 1e-8
    a64 = [normal.clone().requires_grad_(True), light, sv.clone().requires_grad_(True), env.clone().requires_grad_(True)]
    a32 = [t.detach().float().requires_grad_(t.requires_grad) for t in a64]
    ref = (a64[2] * a64[3] * dot(a64[0][:, :, None, :].expand(B, R, M, 3), light, False, eps)).mean(dim=2)
    out = diffuse_light(a32[0], a32[1], a32[2], a32[3], eps)
    assert float((out.detach().double() - ref.detach()).abs().max()) < 2e-6 * max(1.0, float(ref.abs().max()))
    g = torch.tensor(np.random.RandomState(1).randn(B, R, C), dtype=torch.float64, device=gpu)
    gref = torch.autograd.grad(ref, [a64[0], a64[2], a64[3]], g)
    gout = torch.autograd.grad(out, [a32[0], a32[2], a32[3]], g.float())
    for name, go, gr in zip(("normal", "soft_vis", "env"), gout, gref):
        assert float((go.double() - gr).abs().max()) < 2e-5 * max(1.0, float(gr.abs().max())), name


@pytest.mark.parametrize("B,R,M,C", [(1, 40, 128, 1), (2, 7, 32, 3), (1, 3, 200, 1)])
def test_specular_light_matches_composite(gpu, B, R, M, C):
    """fused filament specular integral vs specular_brdf.filament_specular_brdf + renderer.py:155 under autograd (fp64)."""
    from types import SimpleNamespace as NS
    from ndjir_amd.specular_brdf import filament_specular_brdf
    from ndjir_amd.volume import specular_light_filament
    normal, view, light, rough, spec, sv, env = _light_inputs(B, R, M, C, 9 + M, gpu)
    eps, weight = 1e-8, 0.7
    conf = NS(renderer=NS(eps_dot=eps), specular_brdf=NS(sampling="importance"))
    req = (0, 3, 4, 5, 6)
    a64 = [t.clone().requires_grad_(i in req) for i, t in enumerate((normal, view, light, rough, spec, sv, env))]
    a32 = [t.detach().float().requires_grad_(i in req) for i, t in enumerate(a64)]

    def composite(n, v, l, r, s, sv_, e):
        sB, cos = filament_specular_brdf(n, v.reshape(B, R, 1, 3), l, r, s, conf)
        return weight * (sB * sv_ * e * cos).mean(dim=2)

    ref = composite(*a64)
    out = specular_light_filament(*a32, eps, weight)
    stock = composite(*[t.detach().float() for t in a64])
    err = float((out.detach().double() - ref.detach()).abs().max())
    err_stock = float((stock.double() - ref.detach()).abs().max())
    assert err < max(4.0 * err_stock, 1e-6 * max(1.0, float(ref.abs().max()))), (err, err_stock)
    g = torch.tensor(np.random.RandomState(2).randn(B, R, 3), dtype=torch.float64, device=gpu)
    gref = torch.autograd.grad(ref, [a64[i] for i in req], g)
    gout = torch.autograd.grad(out, [a32[i] for i in req], g.float())
    a32s = [t.detach().float().requires_grad_(i in req) for i, t in enumerate(a64)]
    gstock = torch.autograd.grad(composite(*a32s), [a32s[i] for i in req], g.float())
    for name, go, gr, gs in zip(("normal", "roughness", "specular_color", "soft_vis", "env"), gout, gref, gstock):
        scale = max(float(gr.abs().max()), 1e-6)
        e1 = float((go.double() - gr).abs().max()) / scale
        e2 = float((gs.double() - gr).abs().max()) / scale
        assert e1 < max(4.0 * e2, 2e-5), (name, e1, e2)


@pytest.mark.parametrize("shape,M,inc", [((1, 50, 128, 3), 6, True), ((7, 3), 4, True), ((2, 9, 5, 4), 6, False), ((11, 3), 0, True)])
def test_positional_encoding_kernel(gpu, shape, M, inc):
    """fused PE vs the stock-op composite of network.py:96-117 (value and input gradient)."""
    from ndjir_amd.network import positional_encoding
    rng = np.random.RandomState(4)
    x64 = torch.tensor(rng.randn(*shape), dtype=torch.float64, device=gpu, requires_grad=True)
    x32 = x64.detach().float().requires_grad_(True)
    from ndjir_amd.network import _PosEnc
    ref = positional_encoding(x64, M, inc)           # fp64 -> stock ops
    out = _PosEnc.apply(x32, M, inc)                 # the HIP kernel (used by the product for inputs without gradient)
    assert torch.equal(positional_encoding(x32.detach(), M, inc), out.detach())
    assert out.shape == ref.shape
    # |x 2^k| up to ~100: fp32 argument rounding limits cos/sin to ~1e-5
    assert float((out.double() - ref).abs().max()) < 2e-5
    g = torch.tensor(rng.randn(*ref.shape), dtype=torch.float64, device=gpu)
    (gr,) = torch.autograd.grad(ref, x64, g)
    (go,) = torch.autograd.grad(out, x32, g.float())
    assert float((go.double() - gr).abs().max()) < 1e-3 * max(1.0, float(gr.abs().max()))


@pytest.mark.parametrize("remap,entangle,sym", [(True, True, True), (False, False, False), (True, False, True)])
def test_material_head_matches_composite(gpu, remap, entangle, sym):
    """fused output activations + prior integrands vs the stock-op formulas of network.py / loss.py (fp64 autograd)."""
    import torch.nn.functional as TF
    from ndjir_amd.volume import material_head
    B, R, N = 1, 23, 128
    rng = np.random.RandomState(17)
    f = lambda *s: torch.tensor(rng.randn(*s) * 1.5, dtype=torch.float64, device=gpu)
    raws64 = [f(B, R, N, 3), f(B, R, N, 3), f(B, R, N, 1), f(B, R, N, 1), f(B, R, N, 2), f(B, R, N, 6)]
    gain = torch.tensor([1.3], dtype=torch.float64, device=gpu)
    lb, scale, pr, ps = 0.089, 0.16, 0.5, 0.04

    def composite(bc_r, pt_r, imp_r, ph_r, ro_r, sp_r):
        bc, pt = torch.sigmoid(bc_r), torch.sigmoid(pt_r)
        imp, photo = torch.sigmoid(imp_r), torch.sigmoid(gain * ph_r)
        r = torch.sigmoid(ro_r[..., 0:1])
        r = (r ** 2 if remap else r).clamp(lb, 1.0)
        std_r = TF.softplus(ro_r[..., 1:2])
        s = torch.sigmoid(sp_r[..., :3])
        s = 0.16 * s ** 2 if remap else scale * s
        std_s = TF.softplus(sp_r[..., 3:])
        V = torch.cat([imp, r, s, photo, bc * photo if entangle else bc], dim=-1)
        bcp = bc if sym else bc.detach()
        prior = torch.stack([
            (bcp - pt).abs().sum(-1).sum(-1),
            ((r - pr).abs() / std_r).sum(-1).sum(-1),
            torch.log(std_r).clamp(1e-5, 1e5).sum(-1).sum(-1),
            ((s - ps).abs() / std_s).sum(-1).sum(-1),
            torch.log(std_s).clamp(1e-5, 1e5).sum(-1).sum(-1)], dim=-1)
        aux = torch.cat([bc, pt, std_r, std_s], dim=-1)
        return V, aux, prior

    a64 = [t.clone().requires_grad_(True) for t in raws64]
    a32 = [t.float().requires_grad_(True) for t in raws64]
    V64, aux64, pr64 = composite(*a64)
    V32, aux32, pr32 = material_head(a32[0], a32[1], a32[2], a32[3], gain.float(), a32[4], a32[5], remap, entangle, sym,
                                     lb, scale, pr, ps)
    assert float((V32.double() - V64).abs().max()) < 2e-6
    assert float((aux32.double() - aux64).abs().max()) < 1e-5 * max(1.0, float(aux64.abs().max()))
    assert float(((pr32.double() - pr64).abs() / pr64.abs().clamp(min=1.0)).max()) < 2e-5
    gV = torch.tensor(rng.randn(*V64.shape), dtype=torch.float64, device=gpu)
    gp = torch.tensor(rng.randn(*pr64.shape), dtype=torch.float64, device=gpu)
    gref = torch.autograd.grad([V64, pr64], a64, [gV, gp])
    gout = torch.autograd.grad([V32, pr32], a32, [gV.float(), gp.float()])
    for name, go, gr in zip(("base", "ptb", "implicit", "photo", "roughness", "specular"), gout, gref):
        scale_ = max(float(gr.abs().max()), 1e-6)
        assert float((go.double() - gr).abs().max()) / scale_ < 5e-5, name


@pytest.mark.parametrize("entangle", [True, False])
@pytest.mark.parametrize("Ce", [1, 3])
def test_pixel_compose_matches_composite(gpu, entangle, Ce):
    """python/renderer.py:163-178 (fused material head): value and every gradient vs the stock-op composite in fp64."""
    from ndjir_amd.volume import pixel_compose
    g = torch.Generator().manual_seed(3)
    B, R = 2, 37
    mk = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).requires_grad_(True)
    pix, env, spec, bg = mk(B, R, 9), mk(B, R, Ce), mk(B, R, 3), mk(B, R, 3)
    go = torch.randn(B, R, 3, generator=g, dtype=torch.float64)
    imp, photo, base = pix[..., 0:1], pix[..., 5:6], pix[..., 6:9]
    diff = env + imp
    ref = (base * diff + photo * spec if entangle else photo * (base * diff + spec)) + bg
    gref = torch.autograd.grad(ref, [pix, env, spec, bg], go)
    d = [t.detach().float().to(gpu).requires_grad_(True) for t in (pix, env, spec, bg)]
    out = pixel_compose(*d, entangle)
    gout = torch.autograd.grad(out, d, go.float().to(gpu))
    assert float((out.cpu().double() - ref).abs().max()) < 1e-6
    for a, b in zip(gout, gref):
        assert float((a.cpu().double() - b).abs().max()) < 1e-6


@pytest.mark.parametrize("B,R,M,C,acts,ub,entangle,with_bg", [
    (1, 40, 128, 1, ("sigmoid", "softplus"), -1.0, True, True),          # the default configuration
    (2, 7, 32, 3, ("sigmoid", "softplus"), 0.8, False, True),            # RGB light with an upper bound, disentangled
    (1, 5, 200, 1, ("softplus", "relu"), -1.0, True, False),
    (1, 9, 16, 3, ("relu", "sigmoid"), 0.6, True, True)])
def test_direct_light_matches_the_separate_operators(gpu, B, R, M, C, acts, ub, entangle, with_bg):
    """volume.direct_light (output activations of both light nets + diffuse integral + filament specular integral + pixel
    composition, one launch each way) against the fp64 stock-op composite of python/network.py:288-296, 372-376 and
    python/renderer.py:117-178 -- value and the gradient of every differentiable input, incl. the roughness / specular
    columns of pix and the upper-bound clamp."""
    from types import SimpleNamespace as NS
    import torch.nn.functional as TF
    from ndjir_amd.specular_brdf import dot, filament_specular_brdf
    from ndjir_amd.volume import LIGHT_ACTS, direct_light
    rng = np.random.RandomState(M + C)
    normal, view, l_d, _, _, _, _ = _light_inputs(B, R, M, C, 21 + M, gpu)
    _, _, l_s, _, _, _, _ = _light_inputs(B, R, M, C, 22 + M, gpu)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=gpu)
    raw_sv, raw_env = t64(rng.randn(B, R, 2 * M, 1) * 2), t64(rng.randn(B, R, 2 * M, C) * 1.5)
    pix = t64(rng.rand(B, R, 9))
    pix[..., 1] = pix[..., 1] * 0.9 + 0.05
    pix[..., 2:5] *= 0.16
    bg = t64(rng.rand(B, R, 3)) if with_bg else None
    betas = (1.7, 0.6)
    eps, weight = 1e-8, 0.7
    conf = NS(renderer=NS(eps_dot=eps), specular_brdf=NS(sampling="importance"))
    act = {"softplus": lambda v, b: TF.softplus(v, beta=b), "sigmoid": lambda v, b: torch.sigmoid(v), "relu": lambda v, b: torch.relu(v)}
    dirs = torch.cat([l_d, l_s], dim=2)

    def composite(n, rsv, renv, px, bgv):
        sv = act[acts[0]](rsv, betas[0])
        env = act[acts[1]](renv, betas[1])
        if ub > 0:
            env = env.clamp(0.0, ub)
        env_pixel = (sv[:, :, :M] * env[:, :, :M] * dot(n[:, :, None, :].expand(B, R, M, 3), l_d.to(n.dtype), False, eps)).mean(dim=2)
        sB, cos = filament_specular_brdf(n, view.to(n.dtype).reshape(B, R, 1, 3), l_s.to(n.dtype), px[..., 1:2], px[..., 2:5], conf)
        spec = weight * (sB * sv[:, :, M:] * env[:, :, M:] * cos).mean(dim=2)
        imp, photo, base = px[..., 0:1], px[..., 5:6], px[..., 6:9]
        diff = env_pixel + imp
        fg = base * diff + photo * spec if entangle else photo * (base * diff + spec)
        return fg + bgv if bgv is not None else fg

    ins64 = [normal, raw_sv, raw_env, pix] + ([bg] if with_bg else [])
    a64 = [t.clone().requires_grad_(True) for t in ins64]
    ref = composite(*a64, *(() if with_bg else (None,)))
    a32 = [t.detach().float().requires_grad_(True) for t in ins64]
    out = direct_light(a32[0], view.float(), dirs.float(), a32[1], a32[2], a32[3], a32[4] if with_bg else None,
                       (LIGHT_ACTS[acts[0]], LIGHT_ACTS[acts[1]]), (betas[0], betas[1], ub, eps, weight), entangle)
    s32 = [t.detach().float().requires_grad_(True) for t in ins64]
    stock = composite(*s32, *(() if with_bg else (None,)))
    scale = max(1.0, float(ref.abs().max()))
    err, err_stock = float((out.detach().double() - ref.detach()).abs().max()), float((stock.detach().double() - ref.detach()).abs().max())
    assert err < max(4.0 * err_stock, 2e-6 * scale), (err, err_stock)
    g = t64(np.random.RandomState(2).randn(B, R, 3))
    gref = torch.autograd.grad(ref, a64, g)
    gout = torch.autograd.grad(out, a32, g.float())
    gstock = torch.autograd.grad(stock, s32, g.float())
    for name, go, gr, gs in zip(("normal", "raw_soft_vis", "raw_env", "pix", "bg"), gout, gref, gstock):
        sc = max(float(gr.abs().max()), 1e-6)
        e1, e2 = float((go.double() - gr).abs().max()) / sc, float((gs.double() - gr).abs().max()) / sc
        assert e1 < max(4.0 * e2, 2e-5), (name, e1, e2)


def test_gain_matches_composite(gpu):
    """python/network.py:229-231: clip(exp(10 p), 1e-6, 5e4), value and gradient incl. both saturated ends."""
    from ndjir_amd.volume import sdf_gain
    for v in (0.3, -2.0, 1.2, -1.38, 1.08):                     # inside, below lo, above hi, just inside either bound
        p64 = torch.tensor([v], dtype=torch.float64, device=gpu, requires_grad=True)
        ref = torch.exp(p64 * 10).clamp(1e-6, 5e4)
        (gref,) = torch.autograd.grad(ref, p64, torch.tensor([0.7], dtype=torch.float64, device=gpu))
        p32 = torch.tensor([v], dtype=torch.float32, device=gpu, requires_grad=True)
        out = sdf_gain(p32)
        (gout,) = torch.autograd.grad(out, p32, torch.tensor([0.7], device=gpu))
        stock = torch.exp(p32.detach() * 10).clamp(1e-6, 5e4)
        assert float((out.detach() - stock).abs().max()) <= 2e-6 * float(stock), v
        assert float((gout.double() - gref).abs().max()) <= 1e-5 * max(float(gref.abs().max()), 1e-12), v


@pytest.mark.parametrize("B,R,N,nx,F", [(1, 37, 32, 4, 256), (2, 5, 7, 3, 17)])
def test_background_head_matches_composite(gpu, B, R, N, nx, F):
    """volume.background_head vs python/network.py:543-556 spelled with stock ops (fp64 autograd)."""
    import torch.nn.functional as TF
    from ndjir_amd.volume import background_head
    rng = np.random.RandomState(N)
    h = torch.tensor(rng.randn(B, R, N, 1 + F) * 0.05, dtype=torch.float64, device=gpu)
    h[0, 0, 0, 0] = 0.5                                          # beta h > 20: softplus' linear branch
    x = torch.tensor(rng.randn(B, R, N, nx), dtype=torch.float64, device=gpu)
    delta = torch.tensor(rng.rand(B, R, N, 1) * 3, dtype=torch.float64, device=gpu)
    h64 = h.clone().requires_grad_(True)
    density, feature = TF.softplus(h64[..., 0:1], beta=100), h64[..., 1:]
    alpha_ref = 1 - torch.exp(-density * delta)
    inp_ref = torch.cat([x, feature], dim=-1)
    ga = torch.tensor(rng.randn(*alpha_ref.shape), dtype=torch.float64, device=gpu)
    gi = torch.tensor(rng.randn(*inp_ref.shape), dtype=torch.float64, device=gpu)
    (gref,) = torch.autograd.grad([alpha_ref, inp_ref], h64, [ga, gi])
    h32 = h.float().requires_grad_(True)
    alpha, inp = background_head(h32, x.float(), delta.float())
    assert torch.equal(inp, inp_ref.detach().float())
    assert float((alpha.detach().double() - alpha_ref.detach()).abs().max()) < 2e-6
    (gout,) = torch.autograd.grad([alpha, inp], h32, [ga.float(), gi.float()], retain_graph=True)
    assert float((gout.double() - gref).abs().max()) < 2e-5 * float(gref.abs().max())
    # either gradient alone
    (g1,) = torch.autograd.grad(alpha, h32, ga.float())
    assert float(g1[..., 1:].abs().max()) == 0.0 and torch.allclose(g1[..., 0], gout[..., 0])


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("n_tv,shards", [(0, 1), (1, 1), (2, 4)])
def test_loss_terms_match_composite(gpu, l2, n_tv, shards):
    """python/loss.py:59-178 (mask term off): every term, the weighted total and all gradients of the total vs the stock-op
    composite in fp64; global mask sum of a ray-sharded step; bit-reproducible total."""
    from ndjir_amd.volume import LOSS_TERM_NAMES, loss_terms
    g = torch.Generator().manual_seed(11)
    B, R, N = 2, 45, 50
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    color, gt = rnd(B, R, 3).requires_grad_(True), rnd(B, R, 3)
    mask = (torch.rand(B, R, 1, 1, generator=g) > 0.3).double()
    gx = rnd(B, R, N, 3).requires_grad_(True)
    prior = torch.rand(B, R, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    tvs = [torch.rand(B, R, N, D, generator=g, dtype=torch.float64).requires_grad_(True) for D in (4, 24)[:n_tv]]
    w = (0.1, 0.2, 0.3, 1e-2, 1e-3)
    msum_g = mask.sum() * 2.5 if shards > 1 else None
    msum = msum_g if msum_g is not None else mask.sum()
    denorm = msum * N + 1e-5
    err = ((color - gt) ** 2 if l2 else (color - gt).abs()).sum() / (B * R * shards)
    eik = (((gx.pow(2).sum(-1, keepdim=True).sqrt() - 1) * mask) ** 2).sum() / denorm
    tv = sum((t * mask).sum() / denorm for t in tvs) if tvs else torch.zeros((), dtype=torch.float64)
    pm = (prior * mask.reshape(B, R, 1)).sum(dim=(0, 1)) / denorm
    total = err + w[0] * eik + w[1] * tv + w[2] * pm[0] + w[3] * pm[1] + w[4] * pm[3] + w[3] * pm[2] + w[4] * pm[4]
    want = dict(loss=total, loss_rgb=err, loss_eikonal=eik, loss_tv=tv, prior_base_color=pm[0], prior_roughness=pm[1],
                reg_std_roughness=pm[2], prior_specular_reflectance=pm[3], reg_std_specular_reflectance=pm[4])
    gref = torch.autograd.grad(total, [color, gx, prior] + tvs)
    dev = lambda t: t.detach().float().to(gpu)
    c_d, gx_d, pr_d = (dev(t).requires_grad_(True) for t in (color, gx, prior))
    tv_d = [dev(t).requires_grad_(True) for t in tvs]
    terms = loss_terms(c_d, dev(gt), dev(mask), gx_d, pr_d, None if msum_g is None else dev(msum_g), N, 1.0 / (B * R * shards), w, l2, tv_d)
    for i, k in enumerate(LOSS_TERM_NAMES):
        assert float(terms[i]) == pytest.approx(float(want[k]), rel=2e-5, abs=1e-9), k
    gout = torch.autograd.grad(terms[0], [c_d, gx_d, pr_d] + tv_d)
    for a, b in zip(gout, gref):
        assert float((a.cpu().double() - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-12)
    again = loss_terms(c_d, dev(gt), dev(mask), gx_d, pr_d, None if msum_g is None else dev(msum_g), N, 1.0 / (B * R * shards), w, l2, tv_d)
    assert torch.equal(again[:9], terms[:9])


@pytest.mark.parametrize("model", ["filament", "ue4"])
@pytest.mark.parametrize("sampling", ["importance", "uniform"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_specular_light_every_branch_matches_composite(gpu, model, sampling, split, C):
    """csrc/render.hip k_specular_light_g (model x sampling x split sum) against the stock-op composite of
    python/specular_brdf.py:40-199 + python/renderer.py:152-158 evaluated in fp64: forward and every input gradient."""
    from ndjir_amd import config as cfg
    from ndjir_amd.specular_brdf import specular_brdf_model
    from ndjir_amd.volume import specular_light
    import torch.nn.functional as F
    torch.manual_seed(11)
    B, R, M = 2, 5, 37
    conf = cfg.load("default", [f"specular_brdf.model={model}", f"specular_brdf.sampling={sampling}",
                                f"specular_brdf.use_split_sum={split}"])
    n = F.normalize(torch.randn(B, R, 3), dim=-1)
    v = F.normalize(n + 0.7 * torch.randn(B, R, 3), dim=-1)
    l = F.normalize(n[:, :, None, :] + 0.8 * torch.randn(B, R, M, 3), dim=-1)
    l[0, 0, :3] = -l[0, 0, :3]                       # a few directions below the surface: the masks
    rough = torch.rand(B, R, 1) * 0.8 + 0.1
    spec = torch.rand(B, R, 3)
    sv = torch.rand(B, R, M, 1)
    env = torch.rand(B, R, M, C) + 0.1
    eps, weight = conf.renderer.eps_dot, 1.3

    def composite(*a):
        n_, v_, l_, r_, s_, sv_, e_ = a
        sB, cos = specular_brdf_model(n_, v_.reshape(B, R, 1, 3), l_, r_, s_, conf)
        if split:
            return weight * (sv_ * e_).mean(dim=2) * (sB * cos).mean(dim=2)
        return weight * (sB * sv_ * e_ * cos).mean(dim=2)

    a64 = [t.double().requires_grad_(i not in (1, 2)) for i, t in enumerate((n, v, l, rough, spec, sv, env))]
    ref = composite(*a64)
    gout = torch.randn(B, R, 3)
    gref = torch.autograd.grad(ref, [a64[i] for i in (0, 3, 4, 5, 6)], gout.double())
    a32 = [t.to(gpu).requires_grad_(i not in (1, 2)) for i, t in enumerate((n, v, l, rough, spec, sv, env))]
    out = specular_light(*a32, eps, weight, model, sampling, split)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-4, atol=1e-6)
    g = torch.autograd.grad(out, [a32[i] for i in (0, 3, 4, 5, 6)], gout.to(gpu))
    for name, a, b in zip(("normal", "roughness", "specular", "soft_vis", "env"), g, gref):
        scale = float(b.abs().max())
        assert float((a.cpu().double() - b).abs().max()) <= 3e-4 * scale + 1e-7, (name, float((a.cpu().double() - b).abs().max()), scale)
