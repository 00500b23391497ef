"""ISA guard of the polyphase front end's fold kernels (CPU suite; hipcc cross-compiles gfx950 without a GPU), in the manner of
test_isa_regression.py: the product translation unit compiled to device assembly with the flags of build.py.

What only the compiler can take away: pfb_fold_kernel exists for the four sample formats and pfb_ring_kernel for the (format, P)
pairs that ship -- those the measurement kept, (P - 1) * bytes per sample >= 12: complex64 and int16 at P = 4, 8, 16, uint8 and
int8 at P = 8, 16 -- and for no other; none of them uses scratch -- the ring kernel's taps and its ring of the last P segments are indexed by
compile-time constants only (the frame loop is unrolled by P), so they live in registers --; every kernel stores its two
adjacent columns as one 16-byte run, and the ring kernel's unrolled trip holds P stores and P sample loads' worth of work, not
P * P."""
import os
import re

import pytest

from test_isa_regression import CSRC, _asm, _find, _kernels, _mix, _resource

FORMATS = (0, 1, 2, 3)       # complex64, uint8, int8, int16
BYTES = {0: 8, 1: 2, 2: 2, 3: 4}
RING = [(fmt, p) for fmt in FORMATS for p in (4, 8, 16) if (p - 1) * BYTES[fmt] >= 12]


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_pfb")
    return _kernels(_asm(os.path.join(CSRC, "ksa_api.hip"), str(d / "ksa_api.s")))


def _stores16(mix):
    return mix["global_store_dwordx4"] + mix["flat_store_dwordx4"]


def test_fold_kernels_exist_for_every_format_without_scratch(product_asm):
    for fmt in FORMATS:
        body, tail = _find(product_asm, "pfb_fold_kernel<%d>" % fmt)
        assert _resource(tail, "ScratchSize") == 0
        assert _stores16(_mix(body)) >= 1, "the two columns are no longer one 16-byte store"
    assert len([k for k in product_asm if "pfb_fold_kernel<" in k]) == len(FORMATS)


def test_ring_kernels_keep_taps_and_ring_in_registers(product_asm):
    assert len(RING) == 10
    for fmt, p in RING:
        body, tail = _find(product_asm, "pfb_ring_kernel<%d, %d>" % (fmt, p))
        assert _resource(tail, "ScratchSize") == 0, (fmt, p)
        mix = _mix(body)
        assert not [k for k in mix if k.startswith("scratch_")], (fmt, p)
        stores = _stores16(mix)
        assert p <= stores <= 2 * p, (fmt, p, stores)       # one per unrolled frame (a peeled copy at most)
        fmas = sum(v for k, v in mix.items() if re.match(r"v_(pk_)?fma(c|ak|mk)?_f32", k))
        assert fmas >= 1
    assert len([k for k in product_asm if "pfb_ring_kernel<" in k]) == len(RING), "a ring kernel that no engine can launch"
