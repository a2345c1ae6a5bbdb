"""Host side of the MLP chain launches (ndjir_amd/mlp.py): the `ChainCall` record against the C declarations it is turned
into, its choice of entry point, and the per-layer lists `reverse_chain` / `bias_targets` build for a backward-direction
chain.  No launch: CPU tensors, `_packed` replaced by the identity."""
import dataclasses
import os
import re

import pytest
import torch

from ndjir_amd import lib, mlp

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndjir_hip.h")
EX_ONLY = ["side_in2", "side_add", "side_out2", "row_bias", "row_bias_div"]


def _declared(name):
    """Parameter names of `int ndjir_<name>(...)` in the header, without the trailing stream."""
    with open(HEADER) as f:
        m = re.search(r"\bint ndjir_%s\(([^;]*?)\);" % name, f.read(), re.S)
    names = [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]
    assert names[-1] == "stream"
    return names[:-1]


def _call(**kw):
    return mlp.ChainCall(kw.pop("mode", 0), 4, None, 5, 5, 2, [None, None], [None, None], [5, 8], [8, 2], **kw)


def test_fields_are_the_header_parameters_in_order():
    fields = [f.name for f in dataclasses.fields(mlp.ChainCall)]
    assert fields[-3:] == ["kind", "flops", "shape"]
    ex = _declared("mlp_chain_ex")
    assert fields[:-3] == ex and len(ex) == 33
    plain = _declared("mlp_chain")
    assert plain[0] == "bwd" and ["mode"] + plain[1:] == [n for n in ex if n not in EX_ONLY]
    for call in (_call(), _call(row_bias=torch.zeros(2, 8))):
        assert len(call.args()) == len(lib.SIGS[call.entry])
    assert (mlp.ACCUM_Y, mlp.ACCUM_BGRAD, mlp.DEFER_BGRAD, mlp.BLOCKED) == (1, 2, 4, 8)


def test_entry_selection_and_argument_order():
    assert _call().entry == "mlp_chain" and _call(mode=1).entry == "mlp_chain"
    assert _call(row_bias=torch.zeros(2, 8)).entry == "mlp_chain_ex"
    assert _call(mode=1, side_add=[None, None]).entry == "mlp_chain_ex"
    assert _call(mode=2).entry == "mlp_chain_ex"
    # every argument at the position of its name in the declaration; unset per-layer lists as L null entries
    call = _call(mode=1, side_add=[None, None], accum_y=mlp.ACCUM_BGRAD, in_bgrad="in_bgrad", workspace="ws", x_amax="xa")
    got = dict(zip(_declared("mlp_chain_ex"), call.args()))
    assert got["side_in2"] == got["side_out2"] == got["side_add"] == [None, None]
    assert got["side_in"] == got["side_out"] == got["bgrad"] == [None, None] and got["ld_side"] == [0, 0]
    assert got["side_amax"] is None and got["row_bias"] is None and got["row_bias_div"] == 0
    assert (got["mode"], got["P"], got["ldx"], got["K0"], got["L"], got["Ks"], got["Ns"]) == (1, 4, 5, 5, 2, [5, 8], [8, 2])
    assert (got["accum_y"], got["in_bgrad"], got["workspace"], got["x_amax"]) == (2, "in_bgrad", "ws", "xa")
    plain = dict(zip(_declared("mlp_chain"), _call(in_bgrad="in_bgrad", side_amax=["a", "b"]).args()))
    assert plain["bwd"] == 0 and plain["in_bgrad"] == "in_bgrad" and plain["side_amax"] == ["a", "b"] and plain["has_output"] == 1
    assert call.flops == 2.0 * 4 * (5 * 8 + 8 * 2)


P, K0 = 4, 5
NETS = [([2], -1, [0, 1]), ([8, 2], -1, [1, 2]), ([8, 8, 2], -1, [2, 3]), ([8, 8, 2], 0, [2, 3]), ([8, 8, 2], 1, [2, 3])]


@pytest.mark.parametrize("bias", ["none", "fresh", "in_place"])
@pytest.mark.parametrize("widths,skip,steps", [(w, s, n) for w, s, ns in NETS for n in ns])
def test_reverse_chain(monkeypatch, widths, skip, steps, bias):
    monkeypatch.setattr(mlp, "_packed", lambda W, transpose: W)
    L = len(widths)
    A, W, kin = [torch.zeros(P, K0)], [], K0
    for j, n in enumerate(widths):
        W.append(torch.zeros(kin, n))
        kin = n + (K0 if j == skip else 0)
        if j < L - 1:
            A.append(torch.zeros(P, kin))
    amax = torch.zeros(L)
    btgt = {"none": None, "fresh": [None] * L, "in_place": [torch.zeros(n) for n in widths]}[bias]
    lists, deltas, bgrads, skip_step, split = mlp.reverse_chain(A, W, steps, skip, btgt, amax)
    assert lists["L"] == steps and lists["bias"] == [None] * steps
    names = ["Wp", "Ks", "Ns", "side_in", "side_out", "ld_side", "bgrad", "side_amax"]
    assert sorted(lists) == sorted(names + ["L", "bias"]) and all(len(lists[k]) == steps for k in names)
    assert len(deltas) == len(bgrads) == L and deltas[L - 1] is None and bgrads[L - 1] is None
    mlp.ChainCall(1, P, None, 1, widths[-1], **lists)                 # (the lists are keyword arguments of the record)
    for i in range(steps):
        j = L - 1 - i
        step = {k: lists[k][i] for k in names}
        assert step["Wp"] is W[j] and (step["Ks"], step["Ns"]) == (W[j].shape[1], W[j].shape[0])
        if j == 0:      # the net's first layer: nothing below it
            assert (step["side_in"], step["side_out"], step["ld_side"], step["bgrad"], step["side_amax"]) == (None, None, 0, None, None)
            continue
        below, wide = j - 1, A[j].shape[1]
        assert step["side_in"] is A[j] and step["ld_side"] == wide and tuple(step["side_out"].shape) == (P, wide)
        d = deltas[below]
        assert tuple(d.shape) == (P, widths[below]) and d.stride() == (wide, 1)
        assert d.data_ptr() == step["side_out"].data_ptr()
        assert d.untyped_storage().data_ptr() == step["side_out"].untyped_storage().data_ptr()
        assert step["side_amax"].data_ptr() == amax[below:below + 1].data_ptr() and step["side_amax"].numel() == 1
        if bias == "none":
            assert step["bgrad"] is None and bgrads[below] is None
        else:
            assert step["bgrad"] is bgrads[below] and tuple(bgrads[below].shape) == (widths[below],)
            assert (bgrads[below] is btgt[below]) == (bias == "in_place")
    if 0 <= skip and L - 2 - skip < steps:
        assert (skip_step, split) == (L - 2 - skip, widths[skip]) and deltas[skip].shape[1] < A[skip + 1].shape[1]
    else:
        assert (skip_step, split) == (-1, 0)


def test_bias_targets_are_all_or_none():
    t = [torch.zeros(2), torch.zeros(3), torch.zeros(4)]
    got, flag = mlp.bias_targets(t, [True, True, True])
    assert all(a is b for a, b in zip(got, t)) and flag == mlp.ACCUM_BGRAD
    got, flag = mlp.bias_targets(t, [True, False, True])              # only where the gradient is needed
    assert got[0] is t[0] and got[1] is None and got[2] is t[2] and flag == mlp.ACCUM_BGRAD
    assert mlp.bias_targets([t[0], None, t[2]], [True, False, True])[0][2] is t[2]      # (an unneeded layer without a buffer: fine)
    assert mlp.bias_targets([t[0], None, t[2]], [True, True, True]) == ([None] * 3, 0)  # a needed layer without one: none
    assert mlp.bias_targets(t, [False, False, False]) == ([None] * 3, 0)
    assert mlp.bias_targets([], []) == ([], 0)
