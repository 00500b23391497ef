"""What the bindings of the companion libraries share: loading a library with its ABI check and signatures, the sample formats
of the ones that take raw IQ, and the create, lifetime, stream and kernel_info methods of the class over it.  _lib.py binds
libksa.so on its own (it loads eagerly); there is no fallback here either: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import KsaError, FMT_C64, FMT_U8, FMT_S8, FMT_S16

HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = {"c64": FMT_C64, "u8": FMT_U8, "s8": FMT_S8, "s16": FMT_S16}
SAMPLE_DTYPES = {FMT_C64: np.dtype(np.complex64), FMT_U8: np.dtype(np.uint8), FMT_S8: np.dtype(np.int8), FMT_S16: np.dtype(np.int16)}


def format_of(fmt):
    """The sample format as a number: a name of FORMATS in either case, or the number itself (the library checks its range)."""
    if not isinstance(fmt, str):
        return int(fmt)
    if fmt.lower() not in FORMATS:
        raise KsaError("unknown fmt [%s], expected one of %s" % (fmt, "|".join(FORMATS)))
    return FORMATS[fmt.lower()]


def host_iq(samples, fmt):
    """(flat array, sample count) of host input that is not cast: complex64 [n], or for the integer formats [2n] I,Q of exactly
    the format's dtype."""
    a = np.ascontiguousarray(samples)
    if fmt == FMT_C64:
        a = np.ascontiguousarray(a, dtype=np.complex64).reshape(-1)
        return a, a.size
    want = SAMPLE_DTYPES[fmt]
    if a.dtype != want or a.size % 2:
        raise KsaError("process wants [2n] %s I,Q, got %s %s" % (want, a.dtype, a.shape))
    return a.reshape(-1), a.size // 2


class Binding:
    """One companion library: its file beside this module, the prefix of its symbols ("kdc_"), the ABI version the binding
    expects and name -> (restype, argtypes) for every symbol its header declares."""

    def __init__(self, file_name, prefix, abi_version, signatures):
        self.file_name, self.prefix, self.abi_version, self.signatures = file_name, prefix, abi_version, signatures
        self.path = os.path.join(HERE, file_name)
        self._loaded = None

    def load(self, path=None):
        path = self.path if path is None else path
        _lib._preload_torch_hip_runtime()      # every library binds the one HIP runtime torch mapped
        if not os.path.exists(path):
            raise KsaError("%s is missing at %s -- build it with `python __graft_entry__.py` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % (self.file_name, path))
        lib = C.CDLL(path)
        abi = getattr(lib, self.prefix + "abi_version")
        abi.restype = C.c_int
        if abi() != self.abi_version:          # checked first: a stale build is named as such, not as a missing symbol
            raise KsaError("%s has ABI %d, this binding expects %d -- rebuild it (python __graft_entry__.py)"
                           % (path, abi(), self.abi_version))
        for name, (res, args) in self.signatures.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        return lib

    def lib(self):
        """The library, loaded on first use (the spectrum engine alone does not need it)."""
        if self._loaded is None:
            self._loaded = self.load()
        return self._loaded

    def check(self, rc):
        if rc != 0:
            raise KsaError(getattr(self.lib(), self.prefix + "last_error")().decode("utf-8", "replace"))


class Companion:
    """Base of the wrapper classes.  A subclass sets _binding and _info_fields (what k??_kernel_info reports after the
    handle, in order) and its constructor ends in _create, which leaves the library's handle in _h."""
    _binding = None
    _info_fields = ()
    _h = None

    def _create(self, *args, stream=None):
        """k??_create(*args, &handle) through check, the handle into _h, then the stream if one was given."""
        h = C.c_void_p()
        self._binding.check(getattr(self._binding.lib(), self._binding.prefix + "create")(*args, C.byref(h)))
        self._h = h
        if stream is not None:
            self.set_stream(stream)

    def _call(self, name, *args):
        self._binding.check(getattr(self._binding.lib(), self._binding.prefix + name)(self._h, *args))

    def close(self):
        if self._h:
            getattr(self._binding.lib(), self._binding.prefix + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """stream: a hipStream_t as int (torch.cuda.current_stream().cuda_stream) or None."""
        self._call("set_stream", C.c_void_p(stream or 0))

    def synchronize(self):
        self._call("synchronize")

    def kernel_info(self):
        v = [C.c_int32() for _ in self._info_fields]
        self._call("kernel_info", *[C.byref(x) for x in v])
        return dict(zip(self._info_fields, [x.value for x in v]))
