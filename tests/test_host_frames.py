"""CPU side of the batched zeroSpan from host memory (ksa_frames_c64 / _u8, ABI 5): the front end's `frameBatch` key and its
refusals, FileSdr.read_blocks against repeated sdr_read, and the ABI / binding / document agreeing on the new entry points."""
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg


def _k():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.kspecanal")


def _src():
    load_pkg()
    return importlib.import_module("prgs-sdr-kspecanal_amd.sources")


# ------------------------------------------------------------------------------------------------ frameBatch
def test_frame_batch_key_parses_and_defaults_to_one():
    K = _k()
    d = K.handle_args({"cmd.stop": False}, ["zeroSpan", "fftSize", "4096"])
    assert d["frameBatch"] == 1
    d = K.handle_args({"cmd.stop": False}, ["zeroSpan", "FRAMEBATCH", "64", "source", "synth"])
    assert d["frameBatch"] == 64 and d["cmd.stop"] is False


@pytest.mark.parametrize("argv,words", [
    (["zeroSpan", "frameBatch", "0"], ("frameBatch",)),
    (["zeroSpan", "frameBatch", "-3"], ("frameBatch",)),
    (["zeroSpan", "frameBatch", "8", "bUsePSD", "true"], ("frameBatch", "bUsePSD")),
])
def test_frame_batch_refusals_name_the_key(capsys, argv, words):
    K = _k()
    with pytest.raises(SystemExit):
        K.handle_args({"cmd.stop": False}, argv)
    out = capsys.readouterr().out
    for w in words:
        assert w in out, out


def test_frame_batch_one_with_psd_is_accepted():
    K = _k()
    d = K.handle_args({"cmd.stop": False}, ["zeroSpan", "frameBatch", "1", "bUsePSD", "true"])
    assert d["frameBatch"] == 1 and d["bUsePSD"] is True and d["cmd.stop"] is False


# ------------------------------------------------------------------------------------------------ FileSdr.read_blocks
def _capture(tmp_path, nbytes, seed):
    raw = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    path = tmp_path / ("cap%d.bin" % seed)
    raw.tofile(path)
    return str(path)


@pytest.mark.parametrize("length", [2 ** 14, 2 ** 18 + 12345, 3 * 2 ** 18, 1000])
@pytest.mark.parametrize("raw", [True, False])
def test_read_blocks_equals_repeated_sdr_read(tmp_path, length, raw):
    """Byte for byte and value for value, including the power-of-two rounding of a short tail read (K:343) and a capture that
    ends inside the last block (EOF: whole blocks only, the same bytes consumed as sdr_read's partial reads)."""
    K, S = _k(), _src()
    k = 5
    per = 2 * sum(n if n >= 2 ** 18 else int(2 ** np.ceil(np.log2(n)))
                  for n in [2 ** 18] * (length // 2 ** 18) + ([length % 2 ** 18] if length % 2 ** 18 else []))
    for nbytes, whole in ((per * k + 7, k), (per * 3 + per // 2, 3)):
        path = _capture(tmp_path, nbytes, length % 1000 + whole)
        a, b = S.FileSdr(path), S.FileSdr(path)
        shape, dt = ((k, 2 * length), np.uint8) if raw else ((k, length), np.complex64)
        out = np.zeros(shape, dtype=dt)
        got = a.read_blocks(k, length, raw, out)
        want = []
        try:
            for _ in range(k):
                want.append(K.sdr_read(b, length, raw=raw))
        except EOFError:
            pass
        assert got == len(want) == whole
        assert a._pos == b._pos, "bytes consumed differ"
        for i in range(got):
            assert out[i].dtype == want[i].dtype and np.array_equal(out[i], want[i]), i


def test_read_blocks_follows_a_looping_capture(tmp_path):
    K, S = _k(), _src()
    path = _capture(tmp_path, 2 * 4096 * 3 + 100, 11)
    a, b = S.FileSdr(path, loop=True), S.FileSdr(path, loop=True)
    out = np.empty((7, 4096), dtype=np.complex64)
    assert a.read_blocks(7, 4096, False, out) == 7
    for i in range(7):
        assert np.array_equal(out[i], K.sdr_read(b, 4096))
    assert a._pos == b._pos


# ------------------------------------------------------------------------------------------------ ABI 5
def test_abi5_declares_binds_and_documents_the_host_batch_entries():
    load_pkg()
    lib = importlib.import_module("prgs-sdr-kspecanal_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "ksa.h")).read()
    assert int(re.search(r"#define\s+KSA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == lib.ABI_VERSION
    assert re.search(r"#define\s+KSA_FRAME_SLOT_BYTES\s+\(32ll << 20\)", hdr)
    for name in ("ksa_frames_c64", "ksa_frames_u8"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        res, args = lib.SIGNATURES[name]
        assert len(args) == 8 and args[3] is lib._I64 and args[4] is lib._I64
    assert len(lib.SIGNATURES) == 52
    from test_host_cli import integration_blocks
    blocks = integration_blocks()
    assert len(blocks["3"]) >= 2 and "ksa.ksa_frames_c64(" in blocks["3"][1]
    assert "ksaMaxFrames" in blocks["2"][0]
    assert any("ksa.ksa_frames_c64(" in b and "ksa_allreduce_state" in b for b in blocks["5"])
    src = open(os.path.join(ROOT, "prgs-sdr-kspecanal_amd", "csrc", "ksa_api.hip")).read()
    ext = src[src.index('extern "C" {'):]
    body = ext[ext.index("static int frames_host("):]
    body = body[:body.index("\n}\n")]
    assert "DeviceGuard" in body and "hipSetDevice" in body and "getenv" not in body
