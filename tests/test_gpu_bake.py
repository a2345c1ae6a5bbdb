"""Mesh export on the device (ndjir_amd/extract.py, csrc/bake.hip) against fp64 restatements of
python/extract_by_mc.py:144-261: baked vertex textures, the head kernel alone, the environment map's direction lattice,
quantisation and files, and the attributed OBJ files.

Bound of every parity check (the form and constants of tests/test_gpu_extract.py): err <= max(4 ref, 2e-6) with err the
product's distance to the fp64 oracle and ref the fp32 oracle's own distance to it on the same inputs."""
import os

import numpy as np
import pytest
import torch

from oracle import graph as G
from tests import bake_ref as R
from tests.parity_utils import small_conf

pytestmark = pytest.mark.gpu

N = 257                     # two 128-point tiles plus one
LAST = 200                  # first point of the last chunk when chunk = 100
CONFIGS = {
    "default": ("default", []),
    "no_voxel": ("no_voxel", []),
    "relu_base_color": ("default", ["base_color_network.act=relu"]),          # material_nets_raw declines: composite path
    "specular_1ch": ("default", ["specular_reflectance_network.channels=1"]),
}
_CASES = {}


def _conf(key):
    variant, ov = CONFIGS[key]
    return small_conf(grid_size=16, variant=variant, overrides=ov)


def _install(params, gpu):
    from ndjir_amd import network, parameter as P
    P.clear_parameters()
    P.set_device(gpu)
    network.seed(313)
    P.set_parameters({k: v.to(gpu).requires_grad_(k != "photogrammetric-light-network/gain") for k, v in params.items()})


def _net_inputs(c, x, feat, n):
    return torch.cat([x] + ([feat] if c.use_geometric_feature else []) + ([n] if c.use_normal else []), dim=-1)


def _geometry(conf, params, pts, dtype):
    """sdf, feature and normal = d(sdf)/dx of the oracle's geometric net (extract_by_mc.py:151-156)."""
    p = {k: v.to(dtype) for k, v in params.items()}
    x = pts.to(dtype).clone().requires_grad_(True)
    sdf, feat, _ = G.geometric_network(x, p, conf)
    n = torch.autograd.grad(sdf.sum(), x)[0]
    return p, x.detach(), sdf.detach(), feat.detach(), n.detach()


def _raws(conf, p, x, feat, n):
    """Raw (pre-activation) outputs of the four material nets: implicit, base colour, roughness, specular."""
    out = []
    for scope, c, shift in (("implicit-illumination-network", conf.implicit_illumination_network, 0),
                            ("base-color-network", conf.base_color_network, 0),
                            ("roughness-network", conf.roughness_network, 1),
                            ("specular-reflectance-network", conf.specular_reflectance_network, 1)):
        act = torch.relu if c.act == "relu" else G.softplus100
        out.append(G._mlp(p, scope, _net_inputs(c, x, feat, n), G._names(c.layers, shift), act=act))
    return out


def _oracle(conf, params, pts, dtype):
    """The six textures, sdf and normal through the oracle's nets in `dtype`; also the nets' outputs before placement."""
    p, x, sdf, feat, n = _geometry(conf, params, pts, dtype)
    with torch.no_grad():
        if conf.base_color_network.act == "relu":      # the oracle's base-colour net is softplus only: same lines, relu hidden layers
            bc = torch.sigmoid(_raws(conf, p, x, feat, n)[1])
        else:
            bc = G.base_color_network(x, feat, n, p, conf)
        imp = G.implicit_illumination_network(x, feat, n, p, conf)
        r, r_std = G.roughness_network(x, feat, n, p, conf)
        s, s_std = G.specular_reflectance_network(x, feat, n, p, conf)
    outs = [t.numpy() for t in (bc, imp, r, s, r_std, s_std)]
    tex = R.place_textures(*outs)
    tex["sdf"], tex["normal"] = sdf.numpy(), n.numpy()
    return tex, outs


def _rescale_last_layer(params, scope, layers, raw, gain, offset):
    """raw' = gain (raw - mean(raw)) + offset, column by column, through the last layer's weights and bias."""
    name = f"{scope}/affine-{layers - 1:02d}/affine"
    W, b = params[name + "/W"].double(), params[name + "/b"].double()
    gain, offset = torch.as_tensor(gain, dtype=torch.float64), torch.as_tensor(offset, dtype=torch.float64)
    params[name + "/W"] = (W * gain).float()
    params[name + "/b"] = (gain * (b - raw.mean(dim=0)) + offset).float()


def _std_offset(z, k):
    """Offset that puts exactly the k largest entries of z above softplus^-1(1)."""
    top = torch.sort(z.reshape(-1), descending=True)[0]
    return R.STD_ONE - float(top[k - 1] + top[k]) / 2


def _case(key, gpu):
    """Parameters (created by the product, last layers of the material nets rescaled), points and the fp64 / fp32 oracle
    results of one configuration -- computed once, never modified."""
    if key in _CASES:
        return _CASES[key]
    from ndjir_amd import network, parameter as P
    from ndjir_amd.extract import bake_vertex_attributes
    conf = _conf(key)
    P.clear_parameters()
    P.set_device(gpu)
    network.seed(313)
    rng = np.random.RandomState(71)
    pts = torch.from_numpy(rng.uniform(-0.9, 0.9, size=(N, 3)).astype(np.float32))
    with torch.no_grad():
        network.geometric_network(torch.zeros(4, 3, device=gpu), conf)
        for k, p in P.get_parameters().items():
            if k.endswith("feature/F"):          # make the grid matter (tests/test_gpu_extract.py)
                p.mul_(100.0)
    bake_vertex_attributes(pts[:4], conf)        # creates the material nets' parameters
    params = {k: v.detach().cpu().clone() for k, v in P.get_parameters().items()}

    # spread the nets' outputs: base colours over (0.05, 0.95), roughness partly below its lower bound, and exactly ten
    # entries of each std output above 1
    p64, x, _, feat, n = _geometry(conf, params, pts, torch.float64)
    with torch.no_grad():
        raw_imp, raw_bc, raw_r, raw_s = _raws(conf, p64, x, feat, n)
    cs = conf.specular_reflectance_network.channels
    _rescale_last_layer(params, "implicit-illumination-network", conf.implicit_illumination_network.layers, raw_imp,
                        1.5 / raw_imp.std(dim=0), 0.0)
    _rescale_last_layer(params, "base-color-network", conf.base_color_network.layers, raw_bc, 2.0 / raw_bc.std(dim=0), 0.0)
    g = torch.cat([1.5 / raw_r[:, :1].std(dim=0), 1.0 / raw_r[:, 1:].std(dim=0)])
    z = (raw_r - raw_r.mean(dim=0)) * g
    _rescale_last_layer(params, "roughness-network", conf.roughness_network.layers, raw_r, g,
                        [0.0, _std_offset(z[:, 1:], 10)])
    g = torch.cat([1.5 / raw_s[:, :cs].std(dim=0), 1.0 / raw_s[:, cs:].std(dim=0)])
    z = (raw_s - raw_s.mean(dim=0)) * g
    _rescale_last_layer(params, "specular-reflectance-network", conf.specular_reflectance_network.layers, raw_s, g,
                        [0.0] * cs + [_std_offset(z[:, cs:], 10)] * cs)

    # the vertices whose std exceeds 1 go to the end: with chunk = 100 the global maximum of the clipped std textures (1)
    # is then found in the last chunk only
    _, outs = _oracle(conf, params, pts, torch.float64)
    big = (outs[4] > 1).any(axis=1) | (outs[5] > 1).any(axis=1)
    pts = torch.cat([pts[torch.from_numpy(~big)], pts[torch.from_numpy(big)]])
    ref64, outs = _oracle(conf, params, pts, torch.float64)
    ref32, _ = _oracle(conf, params, pts, torch.float32)

    # the case is not vacuous (asserted on the fp64 oracle's values)
    bc, imp, r, s, r_std, s_std = outs
    for std in (r_std, s_std):
        over = (std > 1).any(axis=1)
        assert over.any() and not over.all()
        assert np.nonzero(over)[0].min() >= LAST and std[:LAST].max() < 1
    lb = conf.roughness_network.lower_bound
    assert (r == lb).any() and (r > lb).any()
    assert bc.min() < 0.05 and bc.max() > 0.95
    _CASES[key] = dict(conf=conf, params=params, pts=pts, ref64=ref64, ref32=ref32)
    return _CASES[key]


def _check(got, ref64, ref32, label):
    keys = R.TEXTURES + ("sdf", "normal")
    assert set(keys) <= set(got)
    bad = []
    for k in keys:
        a = got[k].detach().cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert a.shape == ref64[k].shape and a.dtype == np.float32, k
        err = np.abs(a.astype(np.float64) - ref64[k]).max()
        ref = np.abs(ref32[k].astype(np.float64) - ref64[k]).max()
        print(f"{label} {k}: err={err:.3e} ref={ref:.3e}")
        if not err <= max(4 * ref, 2e-6):
            bad.append((k, err, ref))
    assert not bad, bad


@pytest.mark.parametrize("key", list(CONFIGS))
@pytest.mark.parametrize("chunk", [100, 1 << 18])
def test_bake_matches_fp64_oracle(gpu, key, chunk, monkeypatch):
    from ndjir_amd import lib
    from ndjir_amd.extract import bake_vertex_attributes
    c = _case(key, gpu)
    _install(c["params"], gpu)
    launched, call = [], lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (launched.append(name), call(name, *a))[1])
    got = bake_vertex_attributes(c["pts"].numpy() if chunk == 100 else c["pts"], c["conf"], chunk=chunk)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in got.values())
    assert got["sdf"].shape == (N, 1) and got["normal"].shape == (N, 3)
    _check(got, c["ref64"], c["ref32"], f"{key}/chunk={chunk}")
    # the path under test: the stock-op composite for the relu net, the head kernel (once per chunk) otherwise
    chunks = 3 if chunk == 100 else 1
    assert launched.count("bake_head") == (0 if key == "relu_base_color" else chunks)
    assert launched.count("bake_scale") == (0 if key == "relu_base_color" else 1)
    for k in ("roughness_std", "specular_reflectance_std"):
        assert float(got[k].max()) == 1.0
        assert float(got[k][:LAST].max()) < 1.0


@pytest.mark.parametrize("key", list(CONFIGS))
def test_bake_single_vertex_and_none(gpu, key):
    from ndjir_amd.extract import bake_vertex_attributes
    c = _case(key, gpu)
    _install(c["params"], gpu)
    pts = c["pts"][N - 3:N - 2]
    ref64, _ = _oracle(c["conf"], c["params"], pts, torch.float64)
    ref32, _ = _oracle(c["conf"], c["params"], pts, torch.float32)
    _check(bake_vertex_attributes(pts, c["conf"]), ref64, ref32, f"{key}/N=1")
    empty = bake_vertex_attributes(np.zeros((0, 3)), c["conf"])
    assert all(empty[k].shape == (0, 3) for k in R.TEXTURES + ("normal",)) and empty["sdf"].shape == (0, 1)


@pytest.mark.parametrize("ci,cs,act_last,beta,remap", [(1, 3, "sigmoid", 1.0, 1), (3, 1, "softplus", 2.0, 0), (1, 1, "relu", 1.0, 1),
                                                       (3, 3, "softplus", 100.0, 0)])
def test_head_kernel_on_crafted_raws(gpu, ci, cs, act_last, beta, remap):
    """ndjir_bake_head + ndjir_bake_scale alone: saturated inputs, zeros and the clamp thresholds."""
    from ndjir_amd import lib
    from ndjir_amd.extract import _LAST_ACTS
    n, lb, scale = 70, 0.089, 0.5
    rough_lb = float(np.log(np.sqrt(lb) / (1 - np.sqrt(lb)))) if remap else float(np.log(lb / (1 - lb)))     # sigmoid [^2] = lb
    special = [20.0, -20.0, 0.0, R.STD_ONE, rough_lb, np.nextafter(np.float32(R.STD_ONE), np.float32(2)),
               np.nextafter(np.float32(rough_lb), np.float32(-9)), 1.0, 1.0 / beta, 30.0, -104.0]
    rng = np.random.RandomState(17)

    def raw(cols):
        a = rng.uniform(-4, 4, size=(n, cols)).astype(np.float32)
        for c in range(cols):
            a[c:c + len(special), c] = special           # every column sees every special value, on different rows
        return torch.from_numpy(a)

    raw_imp, raw_bc, raw_r, raw_s = raw(ci), raw(3), raw(2), raw(2 * cs)
    tex = torch.full((6, n, 3), float("nan"), device=gpu)
    std_max = torch.zeros(2, device=gpu, dtype=torch.int32)
    half = 33                                             # two calls share std_max, like two chunks
    for a, b in ((0, half), (half, n)):
        lib.call("bake_head", b - a, raw_imp[a:b].to(gpu), raw_bc[a:b].to(gpu), raw_r[a:b].to(gpu), raw_s[a:b].to(gpu), ci, cs,
                 _LAST_ACTS[act_last], beta, remap, lb, scale, [tex[i, a:b] for i in range(6)], std_max)
    assert std_max.view(torch.float32).cpu().tolist() == [1.0, 1.0]
    lib.call("bake_scale", n, tex[4], tex[5], std_max)
    got = dict(zip(R.TEXTURES, tex.cpu().numpy()))
    refs = [R.place_textures(*R.head_outputs(raw_imp.to(dt), raw_bc.to(dt), raw_r.to(dt), raw_s.to(dt), act_last, beta, remap, lb,
                                             scale)) for dt in (torch.float64, torch.float32)]
    bad = []
    for k in R.TEXTURES:
        err = np.abs(got[k].astype(np.float64) - refs[0][k]).max()
        ref = np.abs(refs[1][k].astype(np.float64) - refs[0][k]).max()
        print(f"head {k}: err={err:.3e} ref={ref:.3e}")
        if not err <= max(4 * ref, 2e-6):
            bad.append((k, err, ref))
    assert not bad, bad
    # channels nothing is placed in are exactly 0
    assert (got["roughness"][:, [0, 2]] == 0).all() and (got["roughness_std"][:, [0, 2]] == 0).all()
    if ci == 1:
        assert (got["implicit_illumination"][:, :2] == 0).all()
    if cs == 1:
        assert (got["specular_reflectance"][:, 1:] == 0).all() and (got["specular_reflectance_std"][:, 1:] == 0).all()
    # what the reference clips is exactly 1: std outputs of raw 20 / 30, roughness of raw 20 (sigmoid rounds to 1)
    sat = lambda col: np.nonzero(np.isin(col.numpy(), [20.0, 30.0]))[0]
    assert (got["roughness_std"][sat(raw_r[:, 1]), 1] == 1).all() and len(sat(raw_r[:, 1])) == 2
    for c in range(cs):
        assert (got["specular_reflectance_std"][sat(raw_s[:, cs + c]), c] == 1).all()
    if act_last != "sigmoid":
        ch = 2 if ci == 1 else 0
        assert (got["implicit_illumination"][sat(raw_imp[:, 0]), ch] == 1).all()
    assert (got["roughness"][sat(raw_r[:, 0]), 1] == 1).all()
    assert (got["roughness"][:, 1] >= np.float32(lb)).all() and (got["roughness"][:, 1] == np.float32(lb)).any()
    assert all((got[k] >= 0).all() and (got[k] <= 1).all() for k in R.TEXTURES)


@pytest.mark.parametrize("H", [4, 16])
def test_direction_lattice(gpu, H):
    from ndjir_amd import parameter as P
    from ndjir_amd.extract import environment_map_directions
    P.set_device(gpu)
    got = environment_map_directions(H).cpu().numpy()
    ref = R.envmap_directions(H)
    assert got.shape == (H * 2 * H, 3) and got.dtype == np.float32
    # one fp32 ulp at |v| <= 1: the most a last-bit difference of double sin / cos can move the rounded value
    np.testing.assert_allclose(got.astype(np.float64), ref, rtol=0, atol=2.0 ** -23)
    d = got.reshape(H, 2 * H, 3)
    assert d[0, H // 2, 2] != d[0, H // 2 + 1, 2] and abs(d[0, 0, 2] + 1) < 1e-6         # z follows the column
    np.testing.assert_allclose(d[:, 3, 2], d[0, 3, 2], rtol=0, atol=0)                       # ... and not the row


@pytest.mark.parametrize("mode", ["sigmoid", "normalised", "constant", "mirror_1ch", "rgb"])
def test_envmap_quantize_bytes(gpu, mode):
    from ndjir_amd.extract import quantize_environment_map
    H, W = 4, 8
    C = 3 if mode in ("rgb", "normalised") else 1
    rng = np.random.RandomState(23)
    x = rng.uniform(0, 1, size=(H * W, C)).astype(np.float32)
    if mode == "sigmoid":
        x[:5, 0] = [0.0, 1.0, 0.99999994, 0.5, 1.0 / 255]
    elif mode == "constant":
        x[:] = 0.7
    else:
        x *= 3.7                                   # values beyond 1: only the division by M brings them into range
        x[0, 0], x[1, 0], x[2, 0] = 0.0, x.max(), np.nextafter(x.max(), np.float32(0))
        if mode == "mirror_1ch":
            x[:, 0] = np.sort(x[:, 0])             # increasing along the flattened image: a mirrored row decreases
    img, mm = quantize_environment_map(torch.from_numpy(x).to(gpu), H, W, mode == "sigmoid")
    got = img.cpu().numpy()
    ref = R.envmap_quantize(x, H, W, mode == "sigmoid")
    assert got.dtype == np.uint8 and got.shape == ((H, W, 3) if C == 3 else (H, W))
    np.testing.assert_array_equal(got, ref)
    assert mm.cpu().tolist() == [float(x.min()), float(x.max())]
    if mode == "constant":
        assert (got == 255).all()
    if mode == "normalised":
        assert got[0, 0, 0] == 0 and got[0, 1, 0] == 255 and got.max() == 255
    if mode == "mirror_1ch":
        assert (np.diff(got.astype(int), axis=1) <= 0).all() and got[0, 0] > got[0, -1]
        q = np.clip(x / x.max() * np.float32(255), 0, 255).astype(np.uint8).reshape(H, W)
        np.testing.assert_array_equal(got, q[:, ::-1])
    if mode == "rgb":
        q = np.clip(x / x.max() * np.float32(255), 0, 255).astype(np.uint8).reshape(H, W, 3)
        np.testing.assert_array_equal(got, q)       # the file's RGB is the network's RGB


def test_extract_environment_map(gpu, tmp_path):
    from ndjir_amd import parameter as P
    from ndjir_amd.extract import environment_map_directions, extract_environment_map
    conf = _conf("default")
    P.clear_parameters()
    P.set_device(gpu)
    H = 16
    res = extract_environment_map(str(tmp_path), conf, H=H)          # creates the net's parameters
    params = {k: v.detach().cpu().clone() for k, v in P.get_parameters().items()}
    dirs = environment_map_directions(H).cpu().view(1, 1, H * 2 * H, 3)
    c = conf.environment_light_network
    with torch.no_grad():
        p64 = {k: v.double() for k, v in params.items()}
        h = G.positional_encoding(dirs.double(), c.pe_bands)
        raw = G._mlp(p64, "environment-light-network", h, G._names(c.layers)).reshape(-1, c.channels)
    _rescale_last_layer(params, "environment-light-network", c.layers, raw, 1.0 / raw.std(dim=0), 0.5)      # a map with contrast
    _install(params, gpu)
    res = extract_environment_map(str(tmp_path), conf, H=H)
    with torch.no_grad():
        ref64 = G.environment_light_network(dirs.double(), {k: v.double() for k, v in params.items()}, conf).reshape(-1, c.channels)
        ref32 = G.environment_light_network(dirs, params, conf).reshape(-1, c.channels)
    assert float(ref64.max()) > 2 * float(ref64.min())
    x = res["intensity"].cpu()
    assert x.shape == (H * 2 * H, c.channels)
    err, ref = float((x.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
    print(f"envmap intensity: err={err:.3e} ref={ref:.3e}")
    assert err <= max(4 * ref, 2e-6), (err, ref)
    assert sorted(os.listdir(tmp_path)) == ["environment_map.png", "environment_map_min_max.txt"]
    img = R.decode_png(str(tmp_path / "environment_map.png"))
    assert img.shape == (H, 2 * H) and res["image"].dtype == np.uint8
    np.testing.assert_array_equal(img, res["image"])
    np.testing.assert_array_equal(img, R.envmap_quantize(x.numpy(), H, 2 * H, False))
    assert len(np.unique(img)) > 8
    m, M = x.numpy().min(), x.numpy().max()
    assert (res["min"], res["max"]) == (m, M)
    assert open(tmp_path / "environment_map_min_max.txt").read() == f"min, max = {str(m)}, {str(M)}"


def test_extract_writes_the_attributed_meshes(gpu, tmp_path):
    from ndjir_amd.extract import bake_vertex_attributes, extract
    c = _case("default", gpu)
    _install(c["params"], gpu)
    conf = c["conf"]
    verts = np.array([[0.3, 0.0, -0.1], [-0.2, 0.35, 0.0], [-0.2, -0.3, 0.2], [0.05, 0.0, 0.4]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    last = extract(str(tmp_path), "net", conf, verts, faces)
    objs = [f"net_512grid_raw_{t}_mesh00.obj" for t in R.TEXTURES]
    # seven mesh / image files and the min-max note
    assert sorted(os.listdir(tmp_path)) == sorted(objs + ["environment_map.png", "environment_map_min_max.txt"])
    assert last == f"{tmp_path}/{objs[-1]}"
    assert R.decode_png(str(tmp_path / "environment_map.png")).shape == (256, 512)
    baked = bake_vertex_attributes(verts, conf)
    nrm = baked["normal"].cpu().numpy().astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    for t, name in zip(R.TEXTURES, objs):
        v, col, vn, f, fn = R.parse_obj(str(tmp_path / name))
        np.testing.assert_array_equal(v, verts)
        np.testing.assert_array_equal(col, baked[t].cpu().numpy())
        np.testing.assert_allclose(vn, nrm, rtol=0, atol=2e-7)
        np.testing.assert_array_equal(f, faces + 1)
        np.testing.assert_array_equal(fn, faces + 1)
    assert extract(str(tmp_path), "net", conf, verts, faces, train=True).endswith("net_128grid_raw_specular_reflectance_std_mesh00.obj")


def test_fixme_raises(gpu):
    from ndjir_amd.extract import bake_vertex_attributes
    conf = small_conf(grid_size=16, overrides=["specular_reflectance_network.fixme=true"])
    with pytest.raises(ValueError, match="fixme"):
        bake_vertex_attributes(np.zeros((3, 3), np.float32), conf)
