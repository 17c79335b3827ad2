"""CPU: every __global__ kernel of the convolution family has a row in the fp64 bounds table (tests/conv_bounds.py), so that a new kernel cannot
land without a case that pins it to the reference; plus the bound helpers themselves."""
import os
import re

import torch

import conv_bounds as cb

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "synthanatomy_amd", "csrc")
SOURCES = ("conv_fprop_kernels.h", "conv_wgrad.hip", "conv1.hip", "convt1.hip")

# kernels that are deliberately NOT in the table -- each with the reason
EXCLUDED = {
    # (none: every kernel of these sources is dispatchable and has a bounds case)
}

_GLOBAL = re.compile(r"__global__[^;{}()]*(?:\([^()]*\)[^;{}()]*)*?\bvoid\s+(\w+)\s*\(")


def kernel_names(text: str):
    return sorted(set(_GLOBAL.findall(text)))


def _declared():
    names = {}
    for f in SOURCES:
        with open(os.path.join(CSRC, f)) as fh:
            for n in kernel_names(fh.read()):
                names[n] = f
    return names


def _covered(name: str) -> bool:
    for c in cb.CASES:
        for k in c["kernels"]:
            if k == name or k.startswith(name + "<"):
                return True
    return False


def test_parser_finds_launch_bounded_kernels():
    src = ("template <typename T>\n__global__ __launch_bounds__(NW * 64, NW / 2) void conv_fprop_probe_kernel(const FpropArgs a) {}\n"
           "__global__ void plain_kernel(int n);\nstatic void host_fn(int);\n")
    assert kernel_names(src) == ["conv_fprop_probe_kernel", "plain_kernel"]


def test_every_convolution_kernel_has_a_bounds_case():
    declared = _declared()
    assert len(declared) >= 20, declared      # (the parser still sees the family)
    missing = sorted(f"{n} ({f})" for n, f in declared.items() if n not in EXCLUDED and not _covered(n))
    assert not missing, f"kernels without a row in tests/conv_bounds.py CASES: {missing}"
    stale = sorted(set(EXCLUDED) - set(declared))
    assert not stale, f"exclusions for kernels that no longer exist: {stale}"


def test_case_table_is_well_formed():
    ids = [c["id"] for c in cb.CASES]
    assert len(ids) == len(set(ids))
    for c in cb.CASES:
        assert c["kernels"], c["id"]
        assert c["dt"] in cb.DT and c["fwd"] in cb.DT and c["out"] in cb.DT, c["id"]
        if c["op"] not in ("conv1", "convt1"):
            assert c["N"] >= 2, c["id"]


def test_half_ulp_and_truncation_are_exact():
    v = torch.tensor([1.0, 1.5, 3.0, 2.0 ** -130, 0.0, -7.0], dtype=torch.float64)
    assert cb.half_ulp(v, "bf16").tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -134, 2.0 ** -134, 2.0 ** -6]
    assert cb.half_ulp(v, "f16").tolist()[:3] == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10]
    assert cb.half_ulp(torch.tensor([2.0 ** -20], dtype=torch.float64), "f16").item() == 2.0 ** -25
    assert cb.half_ulp(v, "f32").abs().sum().item() == 0.0
    r = torch.randn(10000).double()         # (fp32 values: one rounding to the 16-bit type, no double rounding through fp32)
    for dt in ("bf16", "f16"):
        rn = r.to(cb.DT[dt]).double()
        assert ((rn - r).abs() <= cb.half_ulp(r.abs(), dt)).all()                    # round to nearest is within half an ulp
        t = cb.truncated(r, dt)
        assert torch.equal(t.to(cb.DT[dt]).double(), t) and (t.abs() <= r.abs()).all()
        assert not cb.check(rn.float(), t, torch.zeros_like(r), dt)[0]               # ... and a truncated reference is not


def test_bound_separates_fp32_accumulation_from_a_dropped_channel():
    """CPU model of what the GPU cases check: an fp32 sum of exact bf16 products passes; the same sum against a reference that lost one
    input channel fails."""
    g = torch.Generator().manual_seed(0)
    x = cb.rounded(torch.randn(2, 64, 6, 7, 9, generator=g), "bf16")
    w = cb.rounded(torch.randn(40, 64, 3, 3, 3, generator=g) * 0.05, "bf16")
    got = torch.nn.functional.conv3d(x, w, padding=1)                       # fp32 accumulation
    x64, w64 = x.double(), w.double()
    ref = torch.nn.functional.conv3d(x64, w64, padding=1)
    A = torch.nn.functional.conv3d(x64.abs(), w64.abs(), padding=1)
    wit = ref - torch.nn.functional.conv3d(x64[:, -1:], w64[:, -1:], padding=1)
    ok, ratio, _ = cb.check(got, ref, A)
    assert ok and ratio < 1e-6, ratio
    assert not cb.check(got, wit, A)[0]
    ok16, _, _ = cb.check(got.to(torch.bfloat16), ref, A, "bf16")
    assert ok16
    assert not cb.check(got.to(torch.bfloat16), cb.truncated(ref, "bf16"), A, "bf16")[0]
