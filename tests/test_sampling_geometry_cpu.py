"""CPU: the launch planner of every sampling geometry (synthanatomy_amd/conv_plan.py, engine.ConvOp._get_plans) against the textbook definition of a
(transposed) convolution, the plans of the default tuples against the plans recorded before the planner existed, and construction / refusals of the
network.  No GPU, no library."""
import json
import os

import pytest
import torch
import torch.nn as nn

from synthanatomy_amd import conv_plan

HERE = os.path.dirname(os.path.abspath(__file__))

# (kind, k, s, p, op, d): the rows of tests/test_sampling_geometry_gpu.py
TUPLES = [("conv", 4, 2, 1, 0, 1), ("conv", 3, 2, 1, 0, 1), ("conv", 2, 2, 0, 0, 1), ("conv", 3, 1, 2, 0, 2),
          ("convT", 4, 2, 1, 1, 1), ("convT", 3, 2, 1, 1, 1), ("convT", 2, 2, 0, 0, 1), ("convT", 3, 1, 2, 0, 2)]
EXTENTS = [(5, 6, 7), (4, 7, 9)]


def _definition(kind, k, s, p, op, d, idims):
    """{(output voxel, tap, input voxel)} from the textbook loops: conv i = o * s - p + t * d, convT o = i * s - p + t * d"""
    odims = tuple(conv_plan.out_size(kind, k, s, p, op, d, i) for i in idims)
    coarse, fine = (odims, idims) if kind == "conv" else (idims, odims)
    res = set()
    for cd in range(coarse[0]):
        for ch in range(coarse[1]):
            for cw in range(coarse[2]):
                c = (cd, ch, cw)
                for tap in range(k ** 3):
                    t = (tap // (k * k), (tap // k) % k, tap % k)
                    f = tuple(c[a] * s - p + t[a] * d for a in range(3))
                    if all(0 <= f[a] < fine[a] for a in range(3)):
                        res.add((c, tap, f) if kind == "conv" else (f, tap, c))      # (output, tap, input)
    return odims, res


@pytest.mark.parametrize("idims", EXTENTS, ids=str)
@pytest.mark.parametrize("tup", TUPLES, ids=str)
def test_plans_enumerate_the_definition_exactly_once(tup, idims):
    kind, k, s, p, op, d = tup
    odims, want = _definition(kind, k, s, p, op, d, idims)
    pl = conv_plan.plan(kind, k, s, p, op, d, idims)
    assert pl["odims"] == odims
    if kind == "convT":      # torch agrees on the output size
        assert tuple(nn.ConvTranspose3d(1, 1, k, s, p, output_padding=op, dilation=d)(torch.zeros(1, 1, *idims)).shape[2:]) == odims
    else:
        assert tuple(nn.Conv3d(1, 1, k, s, p, dilation=d)(torch.zeros(1, 1, *idims)).shape[2:]) == odims
    for what in ("fwd", "wgrad"):          # rows = output voxels, reads = input voxels
        got = list(conv_plan.triples(pl[what]))
        assert len(got) == len(set(got)), f"{what}: a triple is generated twice"
        assert set(got) == want, what
        rows = [(m, c["out_off"], c["out_mult"]) for c in pl[what] for m in [c["grid"]]]
        written = sum(g[0] * g[1] * g[2] for g, _, _ in rows)
        assert written == odims[0] * odims[1] * odims[2], f"{what}: the classes do not partition the output"
    got = list(conv_plan.triples(pl["dgrad"]))   # rows = input voxels, reads = output (gradient) voxels
    assert len(got) == len(set(got))
    assert {(o, tap, i) for i, tap, o in got} == want
    assert sum(c["grid"][0] * c["grid"][1] * c["grid"][2] for c in pl["dgrad"]) == idims[0] * idims[1] * idims[2]     # unread input voxels are rows too (dx = 0)
    for c in pl["fwd"] + pl["dgrad"]:
        assert all(1 <= n <= 4 for n in c["KT"]) and c["KT"][0] * c["KT"][1] * c["KT"][2] <= 64


def _geom_dict(g):
    return dict(N=g.N, grid=[g.Dm, g.Hm, g.Wm], idims=[g.Di, g.Hi, g.Wi], Cin=g.Cin, odims=[g.Do, g.Ho, g.Wo], Cout=g.Cout, cin_valid=g.cin_valid,
                cout_valid=g.cout_valid, KT=list(g.KT), in_mult=list(g.in_mult), tap_step=list(g.tap_step), in_off=list(g.in_off), out_mult=list(g.out_mult),
                out_off=list(g.out_off), Kpad=g.Kpad, CoutPad=g.CoutPad)


def _plan_dict(p):
    return dict(geom=_geom_dict(p.geom), rows=p.rows, red=p.red, ntaps=p.ntaps, lut=list(p.lut) if p.lut is not None else None, s_row=p.s_row, s_red=p.s_red)


@pytest.mark.parametrize("name,kind,k,s,p,idims", [("conv_k4s2p1", "conv", 4, 2, 1, (8, 10, 12)), ("convT_k4s2p1", "convT", 4, 2, 1, (8, 10, 12)),
                                                    ("conv_k3s1p1", "conv", 3, 1, 1, (6, 7, 9))])
def test_default_plans_unchanged(name, kind, k, s, p, idims):
    """tests/golden/conv_plans_default.json: every field of every launch plan (bf16, N = 2, 16 -> 24 channels, gradient stride 24) as ConvOp built them from
    its hard-coded cases before the planner -- the kernels, packed operands and launch counts of the existing configurations follow from these fields."""
    from synthanatomy_amd.engine import ConvOp
    with open(os.path.join(HERE, "golden", "conv_plans_default.json")) as f:
        want = json.load(f)[name]
    cin, cout = 16, 24
    w = torch.zeros((cout, cin, k, k, k) if kind == "conv" else (cin, cout, k, k, k))
    pl = ConvOp(kind, cin, cout, k, s, p, w, None, torch.bfloat16)._get_plans(2, idims, cout, 24)
    assert list(pl["odims"]) == want["odims"]
    for what in ("fwd", "dgrad", "wgrad"):
        got = [_plan_dict(x) for x in pl[what]]
        assert len(got) == len(want[what]), what
        for i, (a, b) in enumerate(zip(got, want[what])):
            for key in b:
                assert a[key] == b[key], f"{name} {what}[{i}].{key}: {a[key]} != {b[key]}"


CONFIGS = {
    "A": dict(down=((4, 2, 1, 1),) * 3, up=((4, 2, 1, 1, 1), (4, 2, 1, 0, 1), (4, 2, 1, 1, 1))),
    "B": dict(down=((3, 2, 1, 1), (2, 2, 0, 1)), up=((2, 2, 0, 0, 1), (3, 2, 1, 1, 1))),
    "C": dict(down=((4, 2, 1, 1), (3, 1, 2, 2)), up=((3, 1, 2, 0, 2), (4, 2, 1, 0, 1))),
}


def _net(down, up):
    from synthanatomy_amd.networks.vqvae.baseline import BaselineVQVAE
    return BaselineVQVAE(n_levels=len(down), downsample_parameters=down, upsample_parameters=up, n_embed=64, embed_dim=16, n_channels=32, n_res_channels=32,
                         n_res_layers=1, compute_dtype=torch.float32)


@pytest.mark.parametrize("cfg", sorted(CONFIGS), ids=str)
def test_network_builds_with_torch_module_shapes(cfg):
    down, up = CONFIGS[cfg]["down"], CONFIGS[cfg]["up"]
    sd = _net(down, up).state_dict()
    n = len(down)
    want = {}
    cin = 1
    for lvl, (k, s, p, d) in enumerate(down):
        width = 32 if lvl == n - 1 else 16
        m = nn.Conv3d(cin, width, k, s, p, dilation=d)
        want[f"encoder.0.{3 * lvl}.weight"], want[f"encoder.0.{3 * lvl}.bias"] = m.weight.shape, m.bias.shape
        cin = width
    i = 1
    for lvl, (k, s, p, op, d) in enumerate(up):
        last = lvl == n - 1
        m = nn.ConvTranspose3d(32 if lvl == 0 else 16, 1 if last else 16, k, s, p, output_padding=op, dilation=d)
        want[f"decoder.0.{i + 1}.weight"], want[f"decoder.0.{i + 1}.bias"] = m.weight.shape, m.bias.shape
        i += 2 if last else 3
    for key, shape in want.items():
        assert key in sd, (key, sorted(sd))
        assert sd[key].shape == shape, (key, sd[key].shape, shape)


@pytest.mark.parametrize("down,needle", [(((1, 2, 0, 1),), "(1, 2, 0, 1)"), (((3, 2, 2, 2),), "(3, 2, 2, 2)"), (((3, 3, 1, 1),), "(3, 3, 1, 1)"),
                                          (((5, 1, 2, 1),), "(5, 1, 2, 1)")], ids=str)
def test_unsupported_tuples_are_refused_by_name(down, needle):
    with pytest.raises(NotImplementedError) as e:
        _net(down, ((4, 2, 1, 0, 1),))
    assert needle in str(e.value) and "downsample_parameters" in str(e.value)
    k, s, p, d = down[0]
    with pytest.raises(NotImplementedError) as e:
        conv_plan.plan("conv", k, s, p, 0, d, (8, 8, 8))
    assert needle in str(e.value)


def test_tuple_torch_rejects_is_a_value_error_naming_the_flag():
    with pytest.raises(ValueError) as e:
        _net(((4, 2, 1, 1),), ((4, 2, 1, 2, 1),))
    assert "(4, 2, 1, 2, 1)" in str(e.value) and "upsample_parameters" in str(e.value) and "output_padding" in str(e.value)
    from synthanatomy_amd.engine import ConvOp
    with pytest.raises(ValueError):
        ConvOp("convT", 8, 8, 4, 2, 1, torch.zeros(8, 8, 4, 4, 4), None, torch.float32, output_pad=2)
