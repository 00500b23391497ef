"""Resource guard of the integrating polyphase spectrometer's fold kernels (CPU suite; hipcc cross-compiles gfx950 without a
GPU), in the manner of test_pfb_isa.py: the product translation unit compiled to device assembly with the flags of build.py and
read through the project's resource listing.

What only the compiler can take away: pfbpsd_fold_kernel exists for the four sample formats and pfbpsd_ring_kernel for the
(format, P) pairs the shipped rule selects (pfbpsd_ring_pays: every format at P = 4, 8, 16, as measured) and for no other; none of
them uses scratch -- the ring form's taps and its ring of the last P segments live in registers --; and the ring form needs no
more VGPRs, and runs at no lower occupancy, than the existing ring kernel of the same (format, P).  uint8 and int8 at P = 4 have
no such sibling (pfb_ring_pays keeps them on the generic kernel): they are held to the int16 ring kernel at P = 4, whose sample
conversion is the longest.  Resources only."""
import os

import pytest

from test_isa_regression import CSRC, _asm, _find, _kernels, _resource
from test_pfb_isa import FORMATS, RING


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_pfbpsd")
    return _kernels(_asm(os.path.join(CSRC, "ksa_api.hip"), str(d / "ksa_api.s")))


def test_block_fold_kernels_exist_for_every_format_without_scratch(product_asm):
    for fmt in FORMATS:
        _, tail = _find(product_asm, "pfbpsd_fold_kernel<%d>" % fmt)
        assert _resource(tail, "ScratchSize") == 0, fmt
        assert _resource(tail, "NumVgprs") <= 32, fmt          # a streaming kernel at full occupancy
    assert len([k for k in product_asm if "pfbpsd_fold_kernel<" in k]) == len(FORMATS)


def test_block_ring_kernels_stay_within_the_ring_kernels_registers(product_asm):
    pairs = [(fmt, p) for fmt in FORMATS for p in (4, 8, 16)]
    for fmt, p in pairs:
        _, tail = _find(product_asm, "pfbpsd_ring_kernel<%d, %d>" % (fmt, p))
        _, sibling = _find(product_asm, "pfb_ring_kernel<%d, %d>" % ((fmt, p) if (fmt, p) in RING else (3, p)))
        assert _resource(tail, "ScratchSize") == 0, (fmt, p)
        assert _resource(tail, "NumVgprs") <= _resource(sibling, "NumVgprs"), (fmt, p)
        assert _resource(tail, "Occupancy") >= _resource(sibling, "Occupancy"), (fmt, p)
    assert len([k for k in product_asm if "pfbpsd_ring_kernel<" in k]) == len(pairs), "a block ring kernel that no engine can launch"
