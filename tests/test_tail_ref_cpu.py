"""CPU checks of tests/tail_ref.py, the references of tests/test_gpu_tail.py: that the "wrapping" shapes really drive the capped
grid-stride kernels through later passes and the RowCol carry (a guard of the test inputs, not a test of the kernels), and that
the loss reference agrees with the project's CPU oracle (oracle/graph.py) and leaves a switched-off term out entirely."""
import numpy as np
import pytest
import torch

from tests import tail_ref as TR


@pytest.mark.parametrize("name", sorted(TR.WRAP_SHAPES))
def test_wrapping_shape_takes_later_passes_and_the_carry(name):
    s = TR.WRAP_SHAPES[name]
    P, W = s["P"], s["W"]
    total = P * W
    assert total >= 2.5 * TR.STRIDE, "at least three passes per thread"
    assert TR.launch_threads(total) == TR.STRIDE, "the launch is capped"
    assert s["largest"] * 4 <= 64e6, "largest array at most 64 MB"
    if not s.get("rowcol", True):
        return                                   # the kernel divides by a constant: nothing but the pass count to arrange
    assert TR.STRIDE % W != 0, "the column must move from pass to pass"
    flat, t, dq, dr, passes, carries, exact = TR.rowcol_walk(P, W)
    print(f"WRAP {name}: P={P} W={W} passes={passes} dq={dq} dr={dr} carries={carries} at_W={exact}")
    assert passes >= 3 and dr > 0 and carries > 0 and exact > 0
    assert np.array_equal(flat, t), "RowCol's (p, c) is the element t of the loop"
    assert flat.size == total and np.array_equal(np.bincount(flat, minlength=total), np.ones(total, dtype=np.int64)), \
        "every element of the P x W rectangle exactly once"


@pytest.fixture(scope="module")
def oracle_step():
    from ndjir_amd.renderer import make_rand
    from ndjir_amd.synthetic import make_rays
    from tests.parity_utils import random_oracle_params, run_oracle_step, small_conf
    torch.set_num_threads(8)
    conf = small_conf(grid_size=8, n_rays=4, variant="default")
    B, R = 1, 4
    camloc, raydir, color = make_rays(B, R)
    inp = dict(camloc=camloc, raydir=raydir, color_gt=color, rand=make_rand(B, R, conf, "cpu"), cos_anneal=torch.tensor([0.6]))
    params = random_oracle_params(conf)
    res = run_oracle_step(conf, params, inp, torch.float64, backward=False)
    return conf, params, inp, res


def test_loss_reference_matches_the_oracle_graph(oracle_step):
    """One small step through oracle/graph.py in fp64 with every weight on; its intermediate tensors -- pixel colour, grad_x,
    the material head's outputs, the sampled TV -- go through tail_ref.loss_terms: every term of the oracle's dictionary."""
    from oracle import graph as G
    conf, params, inp, res = oracle_step
    tr = conf.train
    assert min(tr.eikonal_weight, tr.tv_weight, tr.base_color_prior_weight, tr.roughness_prior_weight,
               tr.specular_reflectance_prior_weight) > 0.0 and tr.mask_weight == 0.0
    out, r = res["out"], res["out"]["render"]
    mask, x_fg = out["mask"], out["x_fg"]
    B, R, N = x_fg.shape[:3]
    s = lambda t: t.detach().sum(dim=(2, 3))
    prior = torch.stack([
        s((r["base_color"] - r["base_color_ptb"]).abs()),
        s((r["roughness"] - conf.roughness_network.prior_value).abs() / r["std_roughness"]),
        s(torch.log(r["std_roughness"]).clamp(1e-5, 1e5)),
        s((r["specular_reflectance"] - conf.specular_reflectance_network.prior_value).abs() / r["std_specular_reflectance"]),
        s(torch.log(r["std_specular_reflectance"]).clamp(1e-5, 1e5))], dim=-1)
    tvs = []
    for name, p in params.items():
        if name.endswith("feature/F"):
            tv = G._TV[name.split("/")[-2]](x_fg.detach().reshape(-1, 3), p.double(), sym_backward=tr.tv_sym_backward)
            tvs.append(tv.detach().reshape(B, R, N, -1))
    assert tvs
    ref = TR.loss_terms(r["color_pixel"], inp["color_gt"].double(), mask, r["grad_x_fg"], prior, tvs, N, 1.0 / (B * R),
                        (tr.eikonal_weight, tr.tv_weight, tr.base_color_prior_weight, tr.roughness_prior_weight,
                         tr.specular_reflectance_prior_weight), tr.rgb_loss == "l2")
    for k in TR.LOSS_TERM_NAMES:
        want = float(out[k])
        assert want != 0.0, k
        # the reference's 1e-5 is the kernel's fp32 constant, the oracle's the double: 1e-5 (1 - 2^-25 ..) / (sum(mask) N) apart
        assert ref["terms"][k] == pytest.approx(want, rel=1e-9), k


def _case(seed=0, B=1, R=6, N=5):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(color=rnd(B, R, 3), color_gt=rnd(B, R, 3), mask=torch.rand(B, R, 1, 1, generator=g), grad_x=rnd(B, R, N, 3),
                prior=torch.rand(B, R, 5, generator=g), tvs=[torch.rand(B, R, N, 4, generator=g)], N=N, inv_rays=1.0 / (B * R))


@pytest.mark.parametrize("off", [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)])
def test_loss_reference_switched_off_terms(off):
    """Weight zero: the term is reported 0, stays out of the total, and its inputs get an exactly zero gradient; a non-finite
    value among a switched-off term's inputs leaves the total finite."""
    c = _case()
    w = [0.1, 0.2, 0.3, 1e-2, 1e-3]
    for k in off:
        w[k] = 0.0
    ref = TR.loss_terms(**c, weights=w, l2=False)
    names = {0: ["loss_eikonal"], 1: ["loss_tv"], 2: ["prior_base_color"], 3: ["prior_roughness", "reg_std_roughness"],
             4: ["prior_specular_reflectance", "reg_std_specular_reflectance"]}
    cols = {2: [0], 3: [1, 2], 4: [3, 4]}
    for k in range(5):
        for n in names[k]:
            assert (ref["terms"][n] == 0.0) == (k in off), n
    if 0 in off:
        assert float(ref["grads"]["grad_x"].abs().max()) == 0.0
    if 1 in off:
        assert float(ref["grads"]["tvs"][0].abs().max()) == 0.0
    for k in (2, 3, 4):
        g = ref["grads"]["prior"][..., cols[k]]
        assert (float(g.abs().max()) == 0.0) == (k in off)
    full = TR.loss_terms(**c, weights=[0.1, 0.2, 0.3, 1e-2, 1e-3], l2=False)
    parts = dict(zip(range(5), [[("loss_eikonal", 0.1)], [("loss_tv", 0.2)], [("prior_base_color", 0.3)],
                                [("prior_roughness", 1e-2), ("reg_std_roughness", 1e-2)],
                                [("prior_specular_reflectance", 1e-3), ("reg_std_specular_reflectance", 1e-3)]]))
    want = full["terms"]["loss"] - sum(wk * full["terms"][n] for k in off for n, wk in parts[k])
    assert ref["terms"]["loss"] == pytest.approx(want, rel=1e-12)
    # poison the inputs of the switched-off terms
    bad = dict(c)
    bad["grad_x"], bad["prior"], bad["tvs"] = c["grad_x"].clone(), c["prior"].clone(), [c["tvs"][0].clone()]
    if 0 in off:
        bad["grad_x"][0, 1, 2, 0] = float("inf")
    if 1 in off:
        bad["tvs"][0][0, 2, 1, 3] = float("nan")
    for k in (2, 3, 4):
        if k in off:
            bad["prior"][0, 3, cols[k][0]] = float("inf")
            bad["prior"][0, 0, cols[k][-1]] = float("nan")
    poisoned = TR.loss_terms(**bad, weights=w, l2=False)
    assert np.isfinite(poisoned["terms"]["loss"]) and poisoned["terms"]["loss"] == ref["terms"]["loss"]
    assert bool(torch.isfinite(poisoned["grads"]["color"]).all())


def test_loss_reference_options():
    """Absent tensors, a global mask sum, N_prior and the upstream scalar do what their names say."""
    c = _case(1)
    w = [0.1, 0.2, 0.3, 1e-2, 1e-3]
    full = TR.loss_terms(**c, weights=w, l2=True)
    none = TR.loss_terms(c["color"], c["color_gt"], c["mask"], None, None, [], c["N"], c["inv_rays"], w, True)
    assert none["terms"]["loss"] == none["terms"]["loss_rgb"] == full["terms"]["loss_rgb"]
    assert none["grads"]["grad_x"] is None and none["grads"]["prior"] is None and none["grads"]["tvs"] == []
    msg = c["mask"].sum() * 2.0
    g = TR.loss_terms(**c, weights=w, l2=True, mask_sum_global=msg)
    assert g["terms"]["loss_eikonal"] == pytest.approx(full["terms"]["loss_eikonal"] / 2.0, rel=1e-5)
    npr = TR.loss_terms(**c, weights=w, l2=True, N_prior=2 * c["N"])
    assert npr["terms"]["prior_roughness"] == pytest.approx(full["terms"]["prior_roughness"] / 2.0, rel=1e-5)
    assert npr["terms"]["loss_eikonal"] == full["terms"]["loss_eikonal"]
    up = TR.loss_terms(**c, weights=w, l2=True, upstream=-2.5)
    for a, b in ((up["grads"]["color"], full["grads"]["color"]), (up["grads"]["grad_x"], full["grads"]["grad_x"]),
                 (up["grads"]["prior"], full["grads"]["prior"]), (up["grads"]["tvs"][0], full["grads"]["tvs"][0])):
        assert torch.allclose(a, -2.5 * b, rtol=1e-14, atol=0.0)
    assert bool((full["gx_mag"] >= full["grads"]["grad_x"].abs() * (1 - 1e-12)).all())


def test_small_references_agree_with_their_stock_spelling():
    """The encoding, its transposed Jacobian and the positional encoding against autograd of the stock-op spelling (fp64)."""
    from oracle import graph as G
    g = torch.Generator().manual_seed(2)
    P, M = 17, 3
    x = torch.randn(P, 3, generator=g)
    f = torch.randn(P, 4, generator=g)
    e = TR.encode(x, M, [f])
    x64 = x.double().requires_grad_(True)
    pe = G.positional_encoding(x64, M)
    assert torch.allclose(e[:, :3 + 6 * M], pe.detach(), rtol=0, atol=1e-15) and torch.equal(e[:, 3 + 6 * M:], f.double())
    g0 = torch.randn(P, 3 + 6 * M + 4, generator=g)
    n, mag, T = TR.normal_from_g0(e.float(), g0, M, [])
    e64 = TR.d(e.float())                                    # the cos / sin the kernel would read
    J = torch.autograd.functional.jacobian(lambda v: G.positional_encoding(v, M), x64.detach()[0:1])[0, :, 0, :]     # (3 + 6M, 3)
    n0 = g0[0, :3 + 6 * M].double() @ J
    assert torch.allclose(n[0], n0, rtol=1e-6, atol=1e-6) and T == 1 + 2 * M and bool((mag >= n.abs() - 1e-12).all())
    nbar = torch.randn(P, 3, generator=g)
    gb = TR.gbar0(e.float(), nbar, M, [f])
    assert torch.allclose(gb[0, :3 + 6 * M], J @ nbar[0].double(), rtol=1e-6, atol=1e-6) and torch.equal(gb[:, 3 + 6 * M:], f.double())
    xc = torch.randn(5, 2, 4, generator=g)
    for inc in (True, False):
        x4 = xc.double().requires_grad_(True)
        ref = G.positional_encoding(x4, M, inc)
        assert torch.allclose(TR.posenc(xc, M, inc), ref.detach().reshape(10, -1), rtol=0, atol=1e-15)
        gg = torch.randn(*ref.shape, generator=g)
        (gx,) = torch.autograd.grad(ref, x4, gg.double())
        got, mag, T = TR.posenc_backward(xc, gg, M, inc)
        assert torch.allclose(got, gx.reshape(10, 4), rtol=1e-12, atol=1e-12) and T == 2 * M + int(inc)
    h = torch.tensor([[0.19, 1.0], [0.21, 2.0], [-1.0, 3.0], [0.0, 4.0]])
    import torch.nn.functional as TF
    assert torch.allclose(TR.softplus100(h[:, 0].double()), TF.softplus(h[:, 0].double(), beta=100), rtol=1e-14, atol=0.0)
