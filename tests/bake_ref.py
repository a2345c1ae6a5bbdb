"""Restatements of python/extract_by_mc.py:187-261 that the mesh-export tests compare the product with: the placement of a
net's output in an RGB triple (`create_rgb_color`), the six textures of `save_attributed_mesh`, the direction lattice and
the quantisation of `extract_environment_map`, and a PNG decoder.  numpy / torch on the CPU only."""
import math
import struct
import zlib

import numpy as np
import torch
import torch.nn.functional as TF

TEXTURES = ("base_color", "implicit_illumination", "roughness", "specular_reflectance", "roughness_std",
            "specular_reflectance_std")


def create_rgb_color(color, dim):
    """extract_by_mc.py:187-194."""
    color = np.clip(color, 0.0, 1.0)
    if dim == -1:
        return color
    rgb = np.zeros((color.shape[0], 3), dtype=color.dtype)
    rgb[:, dim:dim + 1] = color
    return rgb


def place_textures(bc, imp, r, s, r_std, s_std):
    """The six (N, 3) textures from the nets' outputs (extract_by_mc.py:198-216): fill index -1 = RGB, else the channel;
    the std textures are divided by their maximum over the whole array."""
    ci, cs = imp.shape[1], s.shape[1]
    tex = {
        "base_color": create_rgb_color(bc, -1),
        "implicit_illumination": create_rgb_color(imp, 2 if ci == 1 else -1),
        "roughness": create_rgb_color(r, 1),
        "specular_reflectance": create_rgb_color(s, 0 if cs == 1 else -1),
        "roughness_std": create_rgb_color(r_std, 1),
        "specular_reflectance_std": create_rgb_color(s_std, 0 if cs == 1 else -1),
    }
    for k in ("roughness_std", "specular_reflectance_std"):
        tex[k] = tex[k] / tex[k].max()
    return tex


def head_outputs(raw_imp, raw_bc, raw_r, raw_s, act_last, beta, remap, lower_bound, spec_scale):
    """The nets' output activations on raw (pre-activation) torch tensors of any float dtype (python/network.py:262,
    331-334, 455-462, 499-507) -> numpy (bc, imp, r, s, r_std, s_std)."""
    cs = raw_s.shape[1] // 2
    bc = torch.sigmoid(raw_bc)
    imp = {"softplus": lambda v: TF.softplus(v, beta=beta), "relu": torch.relu, "sigmoid": torch.sigmoid}[act_last](raw_imp)
    r = torch.sigmoid(raw_r[:, 0:1])
    s = torch.sigmoid(raw_s[:, :cs])
    if remap:
        r, s = r ** 2, 0.16 * s ** 2
    else:
        s = spec_scale * s
    r = r.clamp(lower_bound, 1.0)
    return tuple(t.numpy() for t in (bc, imp, r, s, TF.softplus(raw_r[:, 1:2]), TF.softplus(raw_s[:, cs:])))


def envmap_directions(H):
    """extract_by_mc.py:227-237, float64 (H * 2H, 3)."""
    W = 2 * H
    thetas = np.linspace(0, np.pi, H)
    phis = np.linspace(-np.pi, np.pi, W)
    the, phi = np.meshgrid(phis, thetas)
    x = np.cos(phi) * np.sin(the)
    y = np.sin(phi) * np.sin(the)
    z = np.cos(the)
    return np.stack([x, y, z], axis=-1).reshape(H * W, 3)


def envmap_quantize(x, H, W, sigmoid_mode):
    """extract_by_mc.py:242-255 on float32 intensities (H * W, C), then what a reader decodes from the written file: the
    writer takes the array as BGR, so three channels come back in the net's order; one channel stays mirrored."""
    x = np.asarray(x, dtype=np.float32)
    M, m = x.max(), x.min()
    if sigmoid_mode:
        d = x * 255.0
    elif m != M:
        d = x / M * 255.0
    else:
        d = 255.0 * np.ones(x.shape)
    C = x.shape[-1]
    d = d.reshape((H, W, 3) if C == 3 else (H, W))
    d = np.clip(d, 0.0, 255.0).astype(np.uint8)[..., ::-1]
    return np.ascontiguousarray(d[..., ::-1] if C == 3 else d)


def decode_png(path):
    """8-bit grey / RGB PNG with filter type 0 on every row -> uint8 (H, W) / (H, W, 3); checks signature and CRCs."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr, tags = 8, b"", None, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        tags.append(tag)
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert tags[0] == b"IHDR" and tags[-1] == b"IEND"
    W, H, depth, ctype, comp, filt, interlace = hdr
    assert (depth, comp, filt, interlace) == (8, 0, 0, 0) and ctype in (0, 2)
    C = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * C)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((H, W, 3) if C == 3 else (H, W))


def parse_obj(path):
    """`v x y z r g b`, `vn x y z`, `f a//a b//b c//c` -> (verts, colors, normals, faces as written (1-based), normal indices)."""
    v, vn, f, fn = [], [], [], []
    for line in open(path):
        t = line.split()
        if t[0] == "v":
            v.append([np.float32(s) for s in t[1:]])
        elif t[0] == "vn":
            vn.append([np.float32(s) for s in t[1:]])
        elif t[0] == "f":
            f.append([int(s.split("//")[0]) for s in t[1:]])
            fn.append([int(s.split("//")[1]) for s in t[1:]])
    v = np.asarray(v, np.float32)
    return v[:, :3], v[:, 3:], np.asarray(vn, np.float32), np.asarray(f), np.asarray(fn)


STD_ONE = math.log(math.e - 1.0)        # softplus(STD_ONE) = 1
