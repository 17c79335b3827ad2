"""CPU: generalized (ReLU) attention, host side -- the constructor and the CLI act or refuse by name, the restatement of tests/generalized_ref.py equals
the rule written out element by element, and header, ctypes table and library agree on the five new entry points."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from generalized_ref import KERNEL_EPS, as_softmax_kernel, attention, generalized_kernel

NEW_SYMBOLS = ["sa_favor_generalized_features_bwd", "sa_favor_generalized_features_fwd", "sa_favor_generalized_project_bwd",
               "sa_favor_generalized_project_features", "sa_favor_generalized_step"]


def _performer(heads=4, **kw):
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer
    o = Ordering("raster_scan", 3, (1, 2, 3, 4), (False,) * 3, (), ())
    return Performer(num_tokens=33, max_seq_len=24, dim=32, depth=2, heads=heads, ordering=o, dim_head=64, local_attn_heads=2, local_window_size=6, **kw)


def test_generalized_attention_constructs_and_marks_every_layer():
    net = _performer(generalized_attention=True)
    assert net.performer.generalized
    assert [l.generalized for l in net._chain.layers] == [True, True] and not any(l._fused_favor() for l in net._chain.layers)
    assert all(m.generalized for m in net.modules() if type(m).__name__ == "SelfAttention")
    soft = _performer()
    assert not soft.performer.generalized and [l.generalized for l in soft._chain.layers] == [False, False]
    # a layer without global heads has nothing generalized to run
    assert [l.generalized for l in _performer(generalized_attention=True, heads=2)._chain.layers] == [False, False]


def test_state_dict_keys_equal_the_softmax_network():
    a, b = _performer(generalized_attention=True).state_dict(), _performer().state_dict()
    assert list(a.keys()) == list(b.keys()) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)


@pytest.mark.parametrize("fn,name", [(nn.GELU(), "GELU"), (nn.Softplus(), "Softplus"), (torch.relu, "relu")])
def test_another_kernel_fn_is_refused_by_name(fn, name):
    with pytest.raises(NotImplementedError, match=rf"kernel_fn={name}\b"):
        _performer(generalized_attention=True, kernel_fn=fn)
    _performer(kernel_fn=fn)           # (the softmax map never looks at it, as upstream)
    _performer(generalized_attention=True, kernel_fn=nn.ReLU(inplace=True))


@pytest.mark.parametrize("flag", ["ff_dropout", "attn_dropout", "emb_dropout"])
def test_dropout_with_generalized_attention_is_refused_with_both_flag_names(flag):
    with pytest.raises(NotImplementedError) as e:
        _performer(generalized_attention=True, **{flag: 0.1})
    assert "generalized_attention" in str(e.value) and flag in str(e.value)
    _performer(generalized_attention=True, **{flag: 0.0})
    _performer(**{flag: 0.1})


@pytest.mark.parametrize("flag", ["ff_dropout", "attn_dropout", "emb_dropout"])
@pytest.mark.parametrize("mode", ["training", "inference", "healing"])
def test_the_cli_refuses_the_combination_before_the_device(tmp_path, monkeypatch, flag, mode):
    import run_transformer
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.runtime import ddp
    monkeypatch.setattr(_ffi, "lib", lambda: (_ for _ in ()).throw(AssertionError("a kernel library call before the refusal")))
    monkeypatch.setattr(ddp, "init_distributed", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the process group before the refusal")))
    argv = ["run", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:2", f"--project_directory={tmp_path}/", "--experiment_name=e",
            f"--mode={mode}", "--generalized_attention=True", f"--{flag}=0.1"]
    with pytest.raises(NotImplementedError) as e:
        run_transformer.run(argv)
    assert "generalized_attention" in str(e.value) and flag in str(e.value)
    # without the dropout flag the run goes on to the device (here: to the first of the two patched calls)
    with pytest.raises(AssertionError, match="the process group before the refusal"):
        run_transformer.run(argv[:-1])


def test_restatement_equals_the_rule_element_by_element():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 5, 64, generator=g, dtype=torch.float64)
    proj = torch.randn(10, 64, generator=g, dtype=torch.float64)
    x[0, 0, 0] = 0.0                       # dd = 0 for every feature: relu(0) + eps
    x[1, 2, 4] = -x[1, 2, 3]               # a row and its mirror image: each feature is positive in exactly one of them (or zero in both)
    phi = generalized_kernel(x, proj)
    assert phi.shape == (2, 3, 5, 10) and phi.dtype == torch.float64
    c = 64 ** -0.25
    for b in range(2):
        for h in range(3):
            for i in range(5):
                for j in range(10):
                    dd = sum(c * float(x[b, h, i, d]) * float(proj[j, d]) for d in range(64))
                    assert abs(float(phi[b, h, i, j]) - (max(dd, 0.0) + 1e-3)) <= 1e-12 * (1.0 + abs(dd)), (b, h, i, j)
    assert KERNEL_EPS == 1e-3 and bool((phi[0, 0, 0] == 1e-3).all())
    pair = torch.minimum(phi[1, 2, 3], phi[1, 2, 4])
    assert bool((pair == 1e-3).all()) and bool((phi >= 1e-3).all())
    # the drop-in for oracle.performer_ref.softmax_kernel ignores is_query
    assert torch.equal(as_softmax_kernel(x, proj, True), phi) and torch.equal(as_softmax_kernel(x, proj, False), phi)
    # attention built from it: position 0 attends to itself only -> v_0 up to the normaliser's eps; every row is a convex-like mix with positive weights
    v = torch.randn(2, 3, 5, 64, generator=g, dtype=torch.float64)
    out = attention(x, x, v, proj)
    w0 = (phi[..., 0, :] * phi[..., 0, :]).sum(-1)
    assert torch.allclose(out[..., 0, :], v[..., 0, :] * (w0 / (w0 + 1e-6 * phi[..., 0, :].sum(-1)))[..., None], rtol=1e-12, atol=0)


def _header_text():
    txt = open(os.path.join(ROOT, "include", "synthanatomy_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_ffi_and_library_agree_on_the_new_entry_points():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    hdr = _header_text()
    declared = sorted(s for s in set(re.findall(r"\b(sa_[a-z0-9_]+)\s*\(", hdr)) if s.startswith("sa_favor_generalized_"))
    assert declared == NEW_SYMBOLS
    assert sorted(s for s in _ffi.declared_symbols() if s.startswith("sa_favor_generalized_")) == NEW_SYMBOLS
    lib = ctypes.CDLL(build(verbose=False))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
        proto = re.search(rf"\bint {s}\s*\(([^;]*)\)\s*;", hdr)
        assert proto, s
        assert len(proto.group(1).split(",")) == len(_ffi._SIGS[s][1]), f"{s}: the ctypes signature and the prototype differ in their argument count"
        assert _ffi._SIGS[s][0] is ctypes.c_int
    assert lib.sa_abi_version() == 5 == _ffi.ABI_VERSION      # additive: the ABI version stays
