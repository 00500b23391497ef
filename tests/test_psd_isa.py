"""ISA guard of the Welch PSD fold (CPU suite; hipcc cross-compiles gfx950 without a GPU), in the manner of
test_isa_regression.py: the product translation unit compiled to device assembly with the flags of build.py.

The PSD fold is a template constant (CM = 4) of every spectrum kernel family.  What only the compiler can take away: the
instantiations exist for both sample formats, none of them holds a v_sqrt_f32 (the fold sums |X|^2; the output stage is AVG's:
sum, scale, no root), and none uses more scratch or reaches a lower occupancy than its AVG sibling -- the ping-pong kernel
spectrum_kernel<4096, c64, RM = 8, PSD> above all (168 VGPRs, three waves per SIMD, no scratch), and spectrum32_kernel<16384>,
whose PSD fold needs a scheduling fence to stay inside AVG's spill budget (ksa_kernels32.hpp)."""
import os
import re

import pytest

from test_isa_regression import CSRC, _asm, _find, _kernels, _mix, _resource

PSD = 4


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_psd")
    return _kernels(_asm(os.path.join(CSRC, "ksa_api.hip"), str(d / "ksa_api.s")))


def _is_psd(name):
    return "mixed_radix_psd_kernel<" in name or re.search(r"spectrum\w*_kernel<[^>]*, %d(, (true|false))?>" % PSD, name) is not None


def _sibling(kernels, name):
    """The kernel the other folds run at the same shape: the AVG constant (CM = 1), or the run-time-fold instantiation (CM = 0)
    where the family has no AVG constant (spectrum_kernel<4096, ., 0, .>; mixed_radix_kernel for mixed_radix_psd_kernel)."""
    if "mixed_radix_psd_kernel<" in name:
        return name.replace("mixed_radix_psd_kernel<", "mixed_radix_kernel<")
    for cm in (1, 0):
        sib = re.sub(r", %d((, (true|false))?>)" % PSD, r", %d\1" % cm, name)
        if sib in kernels:
            return sib
    raise AssertionError("no sibling of " + name)


def _loop_with(body, key, count):
    """The innermost loop holding at least `count` instructions `key`."""
    labels = {m.group(1): m.start() for m in re.finditer(r"^(\.LBB\d+_\d+):", body, flags=re.M)}
    best = None
    for m in re.finditer(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", body, flags=re.M):
        t = m.group(1)
        if t in labels and labels[t] < m.start():
            seg = body[labels[t]:m.start()]
            if _mix(seg)[key] >= count and (best is None or len(seg) < len(best)):
                best = seg
    assert best is not None, "no loop with %d %s" % (count, key)
    return best


def test_psd_instantiations_exist_for_every_family_and_both_formats(product_asm):
    for fmt in (0, 1):
        for needle in ("spectrum_kernel<4096, %d, 8, 4>", "spectrum_kernel<4096, %d, 4, 4>", "spectrum_kernel<4096, %d, 0, 4>",
                       "spectrum_kernel<64, %d, 0, 4>", "spectrum_kernel<16, %d, 0, 4>", "spectrum_kernel<1024, %d, 0, 4>",
                       "spectrum32_kernel<16384, %d, 4>", "spectrum32_kernel<8192, %d, 4>",
                       "spectrum_pair_kernel<1024, %d, 8, 4>", "spectrum_pair_kernel<1024, %d, 0, 4>", "mixed_radix_psd_kernel<%d>"):
            _find(product_asm, needle % fmt)
    for w1 in ("true", "false"):       # the 8 x 8 plan of N = 64 takes complex64 input only
        _find(product_asm, "spectrum64_kernel<0, 4, %s>" % w1)
    # the other folds of the mixed-radix kernel still share one run-time-fold instantiation per format
    for fmt in (0, 1):
        _find(product_asm, "mixed_radix_kernel<%d>" % fmt)


def test_no_psd_kernel_takes_a_square_root_or_falls_behind_its_sibling(product_asm):
    psd = [k for k in product_asm if _is_psd(k)]
    assert len(psd) >= 40, len(psd)
    for name in psd:
        body, tail = product_asm[name]
        assert "v_sqrt_f32" not in body, name
        _, sib_tail = product_asm[_sibling(product_asm, name)]
        got = (_resource(tail, "ScratchSize"), _resource(tail, "Occupancy"))
        sib = (_resource(sib_tail, "ScratchSize"), _resource(sib_tail, "Occupancy"))
        print("%-60s scratch %3d occupancy %d | sibling %3d, %d" % (name[:60], got[0], got[1], sib[0], sib[1]))
        assert got[0] <= sib[0] and got[1] >= sib[1], (name, got, sib)


def test_bench_shapes_psd_siblings(product_asm):
    """The PSD siblings of the three kernels the bench configurations run keep what test_isa_regression.py holds the AVG
    kernels to."""
    # spectrum_kernel<4096, c64 / uint8, RM = 8, PSD>: the ping-pong loop (two windows per trip), no spilled register
    for fmt in (0, 1):
        body, tail = _find(product_asm, "spectrum_kernel<4096, %d, 8, 4>" % fmt)
        assert _resource(tail, "NumVgprs") <= 168 and _resource(tail, "Occupancy") == 3 and _resource(tail, "ScratchSize") == 0
        loop = _mix(_loop_with(body, "ds_read_b64", 64))
        assert loop["ds_read_b64"] == 64 and loop["ds_read2_b64"] + loop["ds_read2st64_b64"] == 0, dict(loop)
        assert loop["s_barrier"] == 8 and not [k for k in loop if k.startswith("scratch_")]
        assert loop["v_mov_b64_e32"] <= 16, "the halves are being moved instead of swapping roles"
        if fmt == 0:
            assert loop["buffer_load_dwordx2"] == 32
    # spectrum64_kernel<c64, PSD>: four waves per SIMD, no scratch, eight 16-byte sample loads per round
    for w1 in ("false", "true"):
        body, tail = _find(product_asm, "spectrum64_kernel<0, 4, %s>" % w1)
        assert _resource(tail, "NumVgprs") <= 128 and _resource(tail, "Occupancy") >= 4 and _resource(tail, "ScratchSize") == 0
        loop = _mix(_loop_with(body, "buffer_load_dwordx4", 8))
        assert loop["buffer_load_dwordx4"] == 8 and loop["ds_read2_b64"] + loop["ds_read2st64_b64"] == 0, dict(loop)
    # spectrum32_kernel<16384, c64, PSD>: AVG's spill budget, no spill store inside the window loop
    body, tail = _find(product_asm, "spectrum32_kernel<16384, 0, 4>")
    assert _resource(tail, "NumVgprs") == 256 and _resource(tail, "Occupancy") == 2 and _resource(tail, "ScratchSize") <= 16
    loop = _mix(_loop_with(body, "ds_read_b64", 64))
    assert not [k for k in loop if k.startswith("scratch_store")]
    assert sum(v for k, v in loop.items() if k.startswith("scratch_load")) <= 4
    assert loop["buffer_load_dwordx4"] == 8 and loop["buffer_load_dwordx2"] == 32
