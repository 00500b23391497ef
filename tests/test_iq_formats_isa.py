"""ISA guard of the int8 / int16 sample formats (CPU suite; hipcc cross-compiles gfx950 without a GPU), in the manner of
test_isa_regression.py: the product translation unit compiled to device assembly with the flags of build.py.

FMT is a template constant of every load stage (0 complex64, 1 uint8, 2 int8, 3 int16).  What only the compiler can take away:
every kernel family has its int8 / int16 instantiations; none of them reaches a lower occupancy than the lower of its complex64
and uint8 siblings or uses more scratch than the larger of the two; and the 50 %-overlap kernel of N = 4096 (the ping-pong loop,
register file full at 168 VGPRs) keeps what the complex64 kernel is held to -- no scratch, three waves per SIMD, single exchange
reads -- with ONE load per sample: as many sample loads in the window loop as the complex64 kernel's buffer_load_dwordx2, each
2 bytes wide (int8) or 4 bytes wide (int16)."""
import os
import re

import pytest

from test_isa_regression import CSRC, _asm, _find, _kernels, _mix, _resource, _window_loop

S8, S16 = 2, 3
# kernel family -> position of FMT among the template arguments
FMT_POS = {"spectrum_kernel": 1, "spectrum_pair_kernel": 1, "spectrum32_kernel": 1, "mixed_radix_kernel": 0,
           "mixed_radix_psd_kernel": 0, "dif16_kernel": 0, "dif_wide_kernel": 0}
MR_FIXED = "mixed_radix_fixed_kernel"      # <FMT, CM>: the int8 / int16 forms of mixed_radix_kernel (CM 0) and mixed_radix_psd_kernel (4)


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_iqfmt")
    return _kernels(_asm(os.path.join(CSRC, "ksa_api.hip"), str(d / "ksa_api.s")))


def _split(name):
    """(family, [template arguments]) of a demangled kernel name, or None for a kernel without a sample format."""
    m = re.search(r"ksa::(\w+)<([^>]*)>", name)
    if not m or (m.group(1) not in FMT_POS and m.group(1) != MR_FIXED):
        return None
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def _fmt_of(name):
    fam, args = _split(name)
    return int(args[0] if fam == MR_FIXED else args[FMT_POS[fam]])


def _with_fmt(name, fmt):
    """The same instantiation for another sample format.  The mixed-radix kernels of int8 / int16 carry a name of their own,
    mixed_radix_fixed_kernel<FMT, 0 | 4>: siblings of mixed_radix_kernel<FMT> (run-time fold) / mixed_radix_psd_kernel<FMT>."""
    fam, args = _split(name)
    args = list(args)
    if fam == MR_FIXED and fmt in (0, 1):
        return re.sub(r"\w+<[^>]*>", "%s<%d>" % ("mixed_radix_psd_kernel" if args[1] == "4" else "mixed_radix_kernel", fmt), name, count=1)
    if fam in ("mixed_radix_kernel", "mixed_radix_psd_kernel") and fmt in (S8, S16):
        return re.sub(r"\w+<[^>]*>", "%s<%d, %d>" % (MR_FIXED, fmt, 4 if fam == "mixed_radix_psd_kernel" else 0), name, count=1)
    args[0 if fam == MR_FIXED else FMT_POS[fam]] = str(fmt)
    return re.sub(r"<[^>]*>", "<" + ", ".join(args) + ">", name, count=1)


def test_every_load_stage_has_its_int8_and_int16_instantiations(product_asm):
    for fmt in (S8, S16):
        for needle in ("spectrum_kernel<16, %d, 0, 1>", "spectrum_kernel<64, %d, 0, 1>", "spectrum_kernel<512, %d, 0, 1>",
                       "spectrum_kernel<1024, %d, 8, 1>", "spectrum_kernel<4096, %d, 8, 1>", "spectrum_kernel<4096, %d, 4, 2>",
                       "spectrum_kernel<4096, %d, 0, 0>", "spectrum_kernel<4096, %d, 8, 4>",
                       "spectrum_pair_kernel<1024, %d, 8, 1>", "spectrum_pair_kernel<1024, %d, 0, 4>",
                       "spectrum32_kernel<8192, %d, 1>", "spectrum32_kernel<16384, %d, 3>", "spectrum32_kernel<16384, %d, 4>",
                       "mixed_radix_fixed_kernel<%d, 0>", "mixed_radix_fixed_kernel<%d, 4>",
                       "dif16_kernel<%d>", "dif_wide_kernel<%d, 32>", "dif_wide_kernel<%d, 64>"):
            _find(product_asm, needle % fmt)
    # the 8 x 8 plan of N = 64 stays complex64-only
    assert not [k for k in product_asm if "spectrum64_kernel<" in k and not "spectrum64_kernel<0," in k]
    # every instantiation that exists for uint8 exists for the two new formats, and nothing else does
    for fmt in (S8, S16):
        mine = {k for k in product_asm if _split(k) and _fmt_of(k) == fmt}
        u8 = {_with_fmt(k, fmt) for k in product_asm if _split(k) and _fmt_of(k) == 1}
        assert mine == u8, sorted(mine ^ u8)[:5]


def test_no_new_instantiation_falls_behind_its_complex64_and_uint8_siblings(product_asm):
    new = [k for k in product_asm if _split(k) and _fmt_of(k) in (S8, S16)]
    assert len(new) >= 160, len(new)
    bad = []
    for name in sorted(new):
        _, tail = product_asm[name]
        sibs = [product_asm[_with_fmt(name, f)][1] for f in (0, 1)]
        got = (_resource(tail, "NumVgprs"), _resource(tail, "ScratchSize"), _resource(tail, "Occupancy"))
        sib = [(_resource(t, "NumVgprs"), _resource(t, "ScratchSize"), _resource(t, "Occupancy")) for t in sibs]
        print("%-58s vgprs %3d scratch %3d occupancy %d | c64 %3d %3d %d | u8 %3d %3d %d"
              % ((name[name.index("ksa::") + 5:name.index("(")][:58],) + got + sib[0] + sib[1]))
        if got[2] < min(s[2] for s in sib) or got[1] > max(s[1] for s in sib):
            bad.append((name, got, sib))
    assert not bad, bad


@pytest.mark.parametrize("fmt,loads", [(S8, ("buffer_load_ushort", "buffer_load_sshort")), (S16, ("buffer_load_dword",))])
def test_config2_shape_kernel_keeps_the_ping_pong_loop_with_one_load_per_sample(product_asm, fmt, loads):
    """spectrum_kernel<4096, int8 / int16, RM = 8, AVG>: what test_isa_regression.py holds the complex64 kernel to, and per
    sample ONE load of the sample's own width."""
    body64, _ = _find(product_asm, "spectrum_kernel<4096, 0, 8, 1>")
    c64_loads = _mix(_window_loop(body64, 32))["buffer_load_dwordx2"]
    assert c64_loads == 32
    body, tail = _find(product_asm, "spectrum_kernel<4096, %d, 8, 1>" % fmt)
    assert _resource(tail, "ScratchSize") == 0 and _resource(tail, "Occupancy") == 3 and _resource(tail, "NumVgprs") <= 168
    loop = _mix(_window_loop(body, 32))
    assert not [k for k in loop if k.startswith("ds_read2")], dict(loop)
    assert loop["ds_read_b64"] == 64 and loop["s_barrier"] == 8, dict(loop)
    assert not [k for k in loop if k.startswith("scratch_")], "scratch traffic inside the window loop"
    assert sum(loop[k] for k in loads) == c64_loads, dict(loop)
    other = [k for k in loop if k.startswith("buffer_load") and k not in loads]
    assert not other, "sample loads of another width in the window loop: %s" % other
    # the unpack is ONE conversion per component (the sign extension is folded into it) and no offset subtraction.  Two windows
    # of 16 samples are 64 conversions at most; the 8 samples the two windows of a trip share need converting once (hipcc reuses
    # them: 48 as of this writing), and the 2 x 8 new samples of a trip at least once.
    conv = sum(v for k, v in loop.items() if k.startswith("v_cvt_f32_i32"))
    assert 32 <= conv <= 64, dict(loop)
    assert not [k for k in loop if k.startswith("v_bfe_i32") or k.startswith("v_ashrrev")], "a separate sign extension: %s" % dict(loop)
    body8, _ = _find(product_asm, "spectrum_kernel<4096, 1, 8, 1>")
    loop8 = _mix(_window_loop(body8, 32))
    valu = lambda m: sum(v for k, v in m.items() if k.startswith("v_"))
    assert valu(loop) <= valu(loop8), (valu(loop), valu(loop8))
