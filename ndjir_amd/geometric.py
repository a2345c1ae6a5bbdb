"""Geometric network main pass: sdf, feature AND n = d(sdf)/dx in fused MFMA chains, with the
hand-derived double backward.

Reference: `sdf, feature, gain = geometric_network(x, conf)` followed by
`grad_x = nn.grad([sdf], [x])[0]` (python/renderer.py:51-52).  The loss depends on grad_x (eikonal
term python/loss.py:68-76, normals renderer.py:55-58/90-91, input of five nets renderer.py:113-127),
so the weight gradients contain second-order terms.  nnabla builds them by differentiating its
backward graph; here they are derived by hand and mapped onto three kinds of fused chains
(ndjir_amd/csrc/mlp.hip):

  forward      A_{j+1} = softplus(A_j W_j + b_j)            (skip: A_4 = [h_3, e] / sqrt 2)
  sdf chain    s_j = (s_{j+1} W_{j+1}^T) * softplus'(z_j)    backward chain seeded with d sdf = 1;
               g_0 = s_0 W_0^T (+ skip part)                 n = J_e(x)^T g_0   (e = PE + grid encoding)
  --- backward, given sdf-bar, feature-bar, n-bar ---
  tangent      g-bar_0 = J_e(x) n-bar;  s-bar_j = g-bar_j W_j;  g-bar_{j+1} = s-bar_j * softplus'(z_j);
               extra_j = beta * s-bar_j * s_j * exp(-beta h_j)      (= s-bar_j * g_{j+1} * softplus''(z_j))
  backward     delta_j = (delta_{j+1} W_{j+1}^T) * softplus'(z_j) + extra_j
  weights      dW_j = A_j^T delta_j + g-bar_j^T s_j ;  dW_last[:, 0] += colsum(g-bar_last) ;  db_j = colsum(delta_j)
  grid         dF = grad_feature(dX[:, 39:43]) + grad_query_grad_feature(n-bar, g_0[:, 39:43])

The grid encoding may be any concatenation of grid-feature families (dense voxel: 4 columns; `triplaneline`:
tri-plane 24 + tri-line 24 columns, python/network.py:124-127); each contributes its slice of e, of g_0 and of dX
through its own five entry points (query, grad_query, grad_query_grad_grad_output, grad_query_grad_feature,
grad_feature).
"""
import math

import torch
from torch.autograd import Function

from . import lib
from .grid_feature import _core
from .mlp import (ACCUM_Y, BLOCKED, ChainCall, WgradJob, WgradSource, _launch_chain, _packed, _Strided, amax_slots, bias_targets, blocked_layout, chain_workspace,
                  engine_state, require_engine, colsum, grad_target, pb, reverse_chain, wgrad, wgrad_group)


TRI_FUSED_MAX_POINTS = 16384      # ndjir_triplaneline_query_encode pays below this many points (see GeometricMain.forward)
_NO_QUERY_ENCODE = bool(__import__("os").environ.get("NDJIR_NO_QUERY_ENCODE"))      # A/B: the voxel query and the input encoding as two launches


def _enc_call(fam, name, P, C, *args):
    """entry point `name` of grid family `fam` (N = P * channels for the dense families)"""
    lib.call(f"{fam.prefix}_{name}", P * C, *args)


_ONES = {}


def _ones(P, dev):
    """(P, 1) of ones: the seed d(sdf) = 1 of the sdf chain (constant, kept per size)"""
    t = _ONES.get((P, dev))
    if t is None:
        if len(_ONES) > 16:
            _ONES.clear()
        t = _ONES[(P, dev)] = torch.ones((P, 1), device=dev, dtype=torch.float32)
    return t


def _sdf_col(W):
    from .network import _sdf_column
    return _sdf_column(W)


class GeometricMain(Function):
    """(x, cfg, *grids, *W, *b) -> sdf (..,1), feature (..,D), n (..,3), Z (.., ldz).
    `cfg` = (M, skip_at, scale, min, max, families, ste): one grid-feature family name per grid tensor; `ste`
    (`voxel.use_ste`, config/ste.yaml): the grid lookups contribute nothing to n = d(sdf)/dx -- the reference's registered
    backward returns (None, None) for them (python/grid_feature/voxel_feature.py:383-399) -- so J_e(x) is the positional
    encoding's Jacobian alone: no grad_query in the forward, no grad_query_grad_* in the backward.
    Z = [x | feature | n | spare columns] is the packed input of the per-sample material nets (cat(x, feature, normal),
    python/network.py:235-263, 300-336, 380-509): `feature` is a view of its columns, and a gradient arriving for Z counts
    for feature and n."""

    @staticmethod
    def forward(ctx, x, cfg, *tensors):
        M, skip_at, scale, min_, max_, fam_names, ste = cfg
        NG = len(fam_names)
        grids, params = list(tensors[:NG]), tensors[NG:]
        fams = [_core.FAMILIES[f] for f in fam_names]
        L = len(params) // 2
        W, b = list(params[:L]), list(params[L:])
        beta = 100.0
        xf = x.detach().reshape(-1, 3).contiguous()
        P = xf.shape[0]
        dev = xf.device
        has_grid = NG > 0
        enc = []                                           # (family, feature, shape args, channels, first column in e)
        col = npe = 3 + 6 * M
        segs = []
        # one dense voxel grid (default / custom / ste): query and encoding in ONE launch, no intermediate (P, D) tensor
        fused_enc = NG == 1 and fams[0].topo == "voxel" and not _NO_QUERY_ENCODE
        # ... and the tri-plane + tri-line pair (triplaneline): both queries and the encoding in one launch
        # (up to TRI_FUSED_MAX_POINTS points: its lane per (point, column) repeats the stencil per channel -- 13 us against 29 at the
        # sampler's 8 192 points, 65 against 52 at 65 536)
        fused_tri = (NG == 2 and fams[0].topo == "triplane" and fams[1].topo == "triline" and not _NO_QUERY_ENCODE
                     and _core.interp_code(fams[0]) == _core.interp_code(fams[1]) and P <= TRI_FUSED_MAX_POINTS)
        for fam, feat in zip(fams, grids):
            fd = feat.detach().contiguous()
            C = fam.channels(fd.shape, None)
            sa = fam.shape_args(fd.shape, None)
            if not (fused_enc or fused_tri):
                vf = torch.empty((P, C), device=dev, dtype=torch.float32)
                _enc_call(fam, fam.fwd, P, C, vf, xf, fd, *sa, min_, max_, 0)
                segs.append(vf)
            enc.append((fam, fd, sa, C, col))
            col += C
        K0 = col
        e = torch.empty((P, K0), device=dev, dtype=torch.float32)          # A_0 = [x, cos, sin, grid features]
        if fused_enc:
            fam, fd, sa, C, _ = enc[0]
            lib.call("voxel_feature_query_encode", P, M, xf, fd, *sa, min_, max_, _core.interp_code(fam), e, K0)
        elif fused_tri:
            (fp, pd, psa, _, _), (fl, ld_, lsa, _, _) = enc
            lib.call("triplaneline_query_encode", P, M, xf, pd, *psa, ld_, *lsa, min_, max_, _core.interp_code(fp), e, K0)
        else:
            lib.call("geo_encode", P, M, xf, len(segs), segs, [t.shape[1] for t in segs], e, K0)

        # ---- forward chain ----
        Ks = [w.shape[0] for w in W]
        Ns = [w.shape[1] for w in W]
        A = [e]
        for j in range(L - 1):
            A.append(torch.empty((P, Ns[j] + (K0 if j == skip_at else 0)), device=dev, dtype=torch.float32))
        # the output y = [sdf | feature] is stored inside Z = [x | feature | n | spare] (csrc/geo.hip): y starts at Z + 2
        D = Ns[-1] - 1
        ldz = (3 + D + 3 + 1 + 3) // 4 * 4
        Z = torch.empty((P, ldz), device=dev, dtype=torch.float32)
        y = _Strided(Z.view(-1)[2:])
        # recorded maxima (operand scales of the f16x3 weight-gradient kernel): am[j] <-> A[j]; sm[j] <-> s_store[j]
        am, sm = amax_slots(dev, L), amax_slots(dev, L)
        # every hidden tensor of the node (A_1.., s, g-bar_1.., extras, deltas) point-blocked where the 128-point-tile kernel runs
        blk = blocked_layout(P, [a.shape[1] for a in A[1:]], xf.is_cuda)
        fl = BLOCKED if blk else 0
        _launch_chain(ChainCall(0, P, e, K0, K0, L, [_packed(w, False) for w in W], [t.detach() for t in b], Ks, Ns,
                                side_out=A[1:] + [None], ld_side=[a.shape[1] for a in A[1:]] + [0], Y=y, ldy=ldz, accum_y=fl,
                                beta=beta, skip_layer=skip_at, skip_scale=scale,
                                side_amax=[am[j + 1:j + 2] for j in range(L - 1)] + [None], x_amax=am[0:1],
                                kind="chain_fwd", shape=f"{P}:geo {K0}-" + "-".join(map(str, Ns))))

        # ---- sdf chain: backward chain seeded with d(sdf) = 1, first step = column 0 of the last layer ----
        ones = _ones(P, dev)
        # s[j] = d sdf / d z_j, j < L-1: the leading columns of s_store[j], which has the width of A[j + 1]
        lists, s, _, bskip, split = reverse_chain(A, W[:-1] + [_sdf_col(W[-1])], L, skip_at, None, sm)
        s_store = lists["side_out"][L - 2::-1] + [None]
        g0 = (torch.empty if bskip >= 0 else torch.zeros)((P, K0), device=dev, dtype=torch.float32)     # (skip layer: assigned, see mlp.FusedMLP.backward)
        _launch_chain(ChainCall(1, P, ones, 1, 1, **lists, Y=g0, ldy=K0, accum_y=(ACCUM_Y if bskip >= 0 else 0) | fl, beta=beta,
                                skip_layer=bskip, skip_scale=scale, skip_split=split, Xskip=g0 if bskip >= 0 else None, ld_xskip=K0,
                                kind="chain_bwd", shape=f"{P}:sdf 1-" + "-".join(map(str, lists["Ns"]))))

        # ---- n = J_e(x)^T g_0 (one launch; it also completes Z and moves the sdf out of it) ----
        gqs, gos = [], []
        for fam, fd, sa, C, c0 in enc:
            if ste:
                break
            go = torch.empty((P, C), device=dev, dtype=torch.float32)
            lib.call("copy_columns", P, C, _Strided(g0[:, c0:]), K0, go, C)
            gq = torch.empty((P, 3), device=dev, dtype=torch.float32)
            _enc_call(fam, "grad_query", P, C, gq, go, xf, fd, *sa, min_, max_, 0, 0)
            gqs.append(gq)
            gos.append(go)
        n = torch.empty((P, 3), device=dev, dtype=torch.float32)
        sdf = torch.empty((P, 1), device=dev, dtype=torch.float32)
        lib.call("geo_normal", P, M, e, K0, g0, K0, len(gqs), gqs, n, Z, ldz, D, sdf)

        ctx.cfg = (M, skip_at, scale, min_, max_, L, tuple(x.shape), fam_names, ste, blk)
        ctx.engine = engine_state()
        ctx.btgt = [grad_target(t) for t in b]       # accumulate-in-place gradient buffers of the biases (mlp.set_grad_buffer)
        ctx.A, ctx.s_store, ctx.s = A, s_store, s
        ctx.am, ctx.sm = am, sm
        ctx.aux = (xf, gos, ldz)
        ctx.save_for_backward(*W, *grids)
        lead = x.shape[:-1]
        Zv = Z.view(lead + (ldz,))
        return sdf.view(lead + (1,)), Zv[..., 3:3 + D], n.view(lead + (3,)), Zv

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sdf, g_feat, g_n, g_Z):
        M, skip_at, scale, min_, max_, L, xshape, fam_names, ste, blk = ctx.cfg
        require_engine(ctx.engine, blk)
        fl = BLOCKED if blk else 0
        saved = ctx.saved_tensors
        W = list(saved[:L])
        grids = list(saved[L:])
        NG = len(grids)
        has_grid = NG > 0
        A, s_store, s = ctx.A, ctx.s_store, ctx.s
        am, sm = ctx.am, ctx.sm
        xf, gos, ldz = ctx.aux
        gm, dm = amax_slots(xf.device, L), amax_slots(xf.device, L)      # recorded maxima of gbar[j] / deltas[j]
        beta = 100.0
        P = xf.shape[0]
        dev = xf.device
        K0 = A[0].shape[1]
        npe = 3 + 6 * M
        Ks = [w.shape[0] for w in W]
        Ns = [w.shape[1] for w in W]
        D = Ns[-1] - 1
        e = A[0]
        gy = torch.empty((P, Ns[-1]), device=dev, dtype=torch.float32)
        nbar = torch.empty((P, 3), device=dev, dtype=torch.float32) if (g_n is not None or g_Z is not None) else None
        gf = g_feat.reshape(P, -1) if g_feat is not None else None
        if gf is not None and gf.stride(1) != 1:
            gf = gf.contiguous()
        lib.call("geo_backward_begin", P, D, g_sdf.reshape(P).contiguous() if g_sdf is not None else None,
                 _Strided(gf) if gf is not None else None, gf.stride(0) if gf is not None else 0,
                 g_n.reshape(P, 3).contiguous() if g_n is not None else None,
                 g_Z.reshape(P, ldz).contiguous() if g_Z is not None else None, ldz, gy, nbar)

        enc = []          # (family, feature, shape args, channels, first column, gradient destination, is caller's buffer)
        col = npe
        for fname, feat in zip(fam_names, grids):
            fam = _core.FAMILIES[fname]
            fd = feat.detach().contiguous()
            C = fam.channels(fd.shape, None)
            buf = _core.get_grad_buffer(feat)
            enc.append((fam, fd, fam.shape_args(fd.shape, None), C, col, buf if buf is not None else torch.zeros_like(fd),
                        buf is not None))
            col += C

        extras = [None] * L
        gbar = [None] * L                 # gbar[j] = adjoint of g_j = d sdf / d A_j  (P, width of A_j)
        col_last = None
        if nbar is not None:
            # ---- g-bar_0 = J_e(x) n-bar ----
            ggos = []
            for (fam, fd, sa, C, c0, gdst, _), go in zip(enc, [] if ste else gos):
                ggo = torch.empty((P, C), device=dev, dtype=torch.float32)
                _enc_call(fam, "grad_query_grad_grad_output", P, C, ggo, nbar, xf, fd, *sa, min_, max_, 0, 0)
                ggos.append(ggo)
                # n depends on the grid directly through the interpolation derivative
                _enc_call(fam, "grad_query_grad_feature", P, C, gdst, nbar, go, xf, *sa, min_, max_, 0, 1)
            if ste:      # J_e(x) without the grid part: zero columns where the grid encodings sit (the kernel takes its row
                ggos = [torch.zeros((P, C), device=dev, dtype=torch.float32) for (_, _, _, C, _, _, _) in enc]   # width from the segments)
            gb0 = torch.empty((P, K0), device=dev, dtype=torch.float32)
            lib.call("geo_gbar0", P, M, e, K0, nbar, len(ggos), ggos, [t.shape[1] for t in ggos], gb0)
            gbar[0] = gb0
            # ---- tangent chain over layers 0..L-2 ----
            T = L - 1
            for l in range(T):                       # g-bar_{l+1} and extra_l have the width of A_{l+1}
                gbar[l + 1] = torch.empty_like(A[l + 1])
                extras[l] = torch.empty_like(A[l + 1])
            col_last = torch.empty((Ns[L - 2],), device=dev, dtype=torch.float32)
            bg = [None] * (T - 1) + [col_last]
            _launch_chain(ChainCall(2, P, gb0, K0, K0, T, [_packed(w, False) for w in W[:T]], [None] * T, Ks[:T], Ns[:T],
                                    side_in=A[1:], side_out=gbar[1:], ld_side=[a.shape[1] for a in A[1:]], bgrad=bg, accum_y=fl,
                                    has_output=0, beta=beta, skip_layer=skip_at, skip_scale=scale, side_in2=s_store[:T],
                                    side_out2=extras[:T], workspace=chain_workspace(dev, bg),
                                    side_amax=[gm[l + 1:l + 2] for l in range(T)], x_amax=gm[0:1], kind="chain_tan",
                                    shape=f"{P}:tan {K0}-" + "-".join(map(str, Ns[:T]))))

        # ---- backward chain with the extra adjoints ----
        need_x = has_grid
        steps = L if need_x else L - 1
        nb = [ctx.needs_input_grad[2 + NG + L + j] for j in range(L)]
        btgt, bg_acc = bias_targets(ctx.btgt, nb)
        lists, deltas, bgrads, bskip, split = reverse_chain(A, W, steps, skip_at, btgt, dm)
        deltas[L - 1] = gy
        side_add = (extras[L - 2::-1] + [None])[:steps]      # in step order: step i produces the delta of layer L-2-i
        skip = bskip >= 0 and need_x
        gx = (torch.empty if bskip >= 0 else torch.zeros)((P, K0), device=dev, dtype=torch.float32) if need_x else None
        gb_last = btgt[L - 1] if btgt[L - 1] is not None else torch.empty((Ns[-1],), device=dev, dtype=torch.float32)     # bias gradient of the output layer
        _launch_chain(ChainCall(1, P, gy, Ns[-1], Ns[-1], **lists, Y=gx, ldy=K0, accum_y=(ACCUM_Y if skip else 0) | bg_acc | fl,
                                has_output=1 if need_x else 0, beta=beta, skip_layer=bskip, skip_scale=scale, skip_split=split,
                                Xskip=gx if skip else None, ld_xskip=K0, side_add=side_add, in_bgrad=gb_last,
                                workspace=chain_workspace(dev, lists["bgrad"] + [gb_last]), x_amax=dm[L - 1:L], kind="chain_bwd",
                                shape=f"{P}:geo {Ns[-1]}-" + "-".join(map(str, lists["Ns"]))))

        for fam, fd, sa, C, c0, gdst, _ in enc:
            gxc = torch.empty((P, C), device=dev, dtype=torch.float32)
            lib.call("copy_columns", P, C, _Strided(gx[:, c0:]), K0, gxc, C)
            _enc_call(fam, "grad_feature", P, C, gdst, gxc, xf, *sa, min_, max_, 0, 1)

        # ---- weight / bias gradients ----
        gW, gb = [None] * L, [None] * L
        jobs = []           # dW_j = A_j^T delta_j + gbar_j^T s_j: two operand pairs per output, all layers in one grouped launch
        for j in range(L):
            if ctx.needs_input_grad[2 + NG + j]:
                wt = grad_target(W[j])           # accumulate-in-place gradient buffer of the weight, if registered
                dst = wt if wt is not None else torch.empty(tuple(W[j].shape), device=dev, dtype=torch.float32)
                if wt is None:
                    gW[j] = dst
                src = [WgradSource(pb(A[j], blk and j > 0), pb(deltas[j], blk and j < L - 1), am[j:j + 1], dm[j:j + 1])]
                if nbar is not None and j < L - 1:
                    src.append(WgradSource(pb(gbar[j], blk and j > 0), pb(s[j], blk), gm[j:j + 1], sm[j:j + 1]))
                jobs.append(WgradJob(dst, wt is not None, src))
        wgrad_group(jobs)
        for j in range(L):
            if ctx.needs_input_grad[2 + NG + j] and nbar is not None and j == L - 1:
                dst = grad_target(W[j]) if gW[j] is None else gW[j]
                dst[:, 0] += col_last
            if ctx.needs_input_grad[2 + NG + L + j] and btgt[j] is None:
                gb[j] = bgrads[j] if j < L - 1 else gb_last
        g_grids = [gdst if (ctx.needs_input_grad[2 + k] and not own) else None
                   for k, (_, _, _, _, _, gdst, own) in enumerate(enc)]
        ctx.A = ctx.s_store = ctx.s = ctx.aux = ctx.am = ctx.sm = None
        return (None, None, *g_grids, *gW, *gb)


def geometric_main(x, grids, weights, biases, M, skip_at, scale, min_=(-1, -1, -1), max_=(1, 1, 1), use_ste=False):
    """grids: None, one dense-voxel feature tensor, or a list of (family name, feature tensor) in the order their
    outputs are concatenated behind the positional encoding."""
    if grids is None:
        grids = []
    elif torch.is_tensor(grids):
        grids = [("voxel", grids)]
    cfg = (int(M), int(skip_at), float(scale), tuple(min_), tuple(max_), tuple(f for f, _ in grids), bool(use_ste))
    return GeometricMain.apply(x, cfg, *[t for _, t in grids], *weights, *biases)
