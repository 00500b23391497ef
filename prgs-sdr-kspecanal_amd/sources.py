"""IQ sources behind d['sdr'] -- the device seam of the reference (python/kspecanal.py:13-14, :281-308).

The reference duck-types `rtlsdr.RtlSdr`: attributes sample_rate / center_freq / gain /
valid_gains_db / bandwidth / freq_correction, methods read_samples(n) -> complex ndarray and close().
Anything with that surface can be plugged in.  Two sources ship here because the GPU box has no
dongle: a synthetic tone generator (the role of the reference's python/testfft.py, written for
numpy >= 2) and a reader for raw `rtl_sdr` uint8 captures (octave/load_rtlsdr.m:8-12,
octave/hkvc-dump_samples.sh:6).  Both can hand over uint8 I,Q pairs (`read_bytes`) so that the unpack
runs on the GPU (row A0).  Captures also come as interleaved signed int8 (HackRF, SigMF ci8: b / 128) and little-endian
int16 (USRP, SigMF ci16_le, Airspy, SDRplay: b / 32768): `read_iq(n, fmt)` hands those over in their own dtype, again for
the GPU to unpack.
"""
import numpy as np

# iqFormat -> (dtype of one I or Q value, the unpack to [-1, 1): (b - offset) / scale)
IQ_FORMATS = {"u8": (np.dtype(np.uint8), 127.5, 127.5), "s8": (np.dtype(np.int8), 0.0, 128.0),
              "s16": (np.dtype("<i2"), 0.0, 32768.0)}


def quantise(x, fmt):
    """Complex samples -> interleaved I,Q in the capture format `fmt`: clip(round((x+1)*127.5)) as the dongle delivers them,
    clip(round(x*127), -128, 127) for s8, clip(round(x*32767), -32768, 32767) for s16."""
    dtype = IQ_FORMATS[fmt][0]
    out = np.empty(2 * len(x), dtype=dtype)
    for part, v in ((0, x.real), (1, x.imag)):
        if fmt == "u8":
            out[part::2] = np.clip(np.round((v + 1.0) * 127.5), 0, 255)
        elif fmt == "s8":
            out[part::2] = np.clip(np.round(v * 127), -128, 127)
        else:
            out[part::2] = np.clip(np.round(v * 32767), -32768, 32767)
    return out


def unpack(b, fmt):
    """Interleaved I,Q of format `fmt` (last axis) -> complex128, the documented unpack of that format."""
    _, offset, scale = IQ_FORMATS[fmt]
    b = b.astype(np.float64)
    return (b[..., 0::2] - offset) / scale + 1j * ((b[..., 1::2] - offset) / scale)


class _SdrBase:
    valid_gains_db = [0.0, 0.9, 1.4, 2.7, 3.7, 7.7, 8.7, 12.5, 14.4, 15.7, 16.6, 19.7, 20.7, 22.9, 25.4,
                      28.0, 29.7, 32.8, 33.8, 36.4, 37.2, 38.6, 40.2, 42.1, 43.4, 43.9, 44.5, 48.0, 49.6]
    bandwidth = 0
    freq_correction = 0

    def __init__(self):
        self.sample_rate = 2.4e6
        self.center_freq = 92e6
        self.gain = 19.1

    def close(self):
        pass


class SyntheticSdr(_SdrBase):
    """Complex tones at every whole MHz that falls inside the tuned band (amplitude 0.1 .. 0.9 by MHz
    index) plus complex Gaussian noise; deterministic for a seed.  Levels follow the reference fake's
    convention of scaling by 10**(gain/10) (python/testfft.py:63) relative to its default gain."""

    def __init__(self, seed=20201226, noise=0.01, ref_gain=19.1):
        super().__init__()
        self._rng = np.random.default_rng(seed)
        self.noise = noise
        self.ref_gain = ref_gain
        self._t0 = 0

    def read_samples(self, n):
        n = int(n)
        fs, fc = float(self.sample_rate), float(self.center_freq)
        t = (self._t0 + np.arange(n, dtype=np.float64)) / fs
        self._t0 += n
        x = np.zeros(n, dtype=np.complex128)
        lo, hi = fc - fs / 2, fc + fs / 2
        for mhz in range(int(np.ceil(lo / 1e6)), int(np.floor(hi / 1e6)) + 1):
            f = mhz * 1e6
            if lo <= f < hi:
                x += (0.1 + 0.1 * (mhz % 9)) * np.exp(2j * np.pi * (f - fc) * t)
        x *= 0.25 * 10 ** ((float(self.gain) - self.ref_gain) / 10)
        x += self.noise * (self._rng.standard_normal(n) + 1j * self._rng.standard_normal(n))
        return x

    def read_bytes(self, nbytes):
        """uint8 I,Q interleaved, as the dongle delivers them (clip(round((x+1)*127.5)))."""
        return quantise(self.read_samples(int(nbytes) // 2), "u8")

    def read_iq(self, n, fmt):
        """n samples as interleaved I,Q of format `fmt` (u8 | s8 | s16), 2*n values of that format's dtype."""
        return quantise(self.read_samples(int(n)), fmt)


class FileSdr(_SdrBase):
    """Replays a raw `rtl_sdr -n ... file.bin` capture: interleaved uint8 I,Q -- or, with iq_format s8 / s16, a capture of
    interleaved signed int8 / little-endian int16 I,Q.  read_samples applies the documented unpack ((b - 127.5)/127.5, b / 128,
    b / 32768); read_bytes hands the file's bytes over untouched and read_iq the same bytes in the format's dtype, for the GPU
    unpack.  At end of file it raises EOFError (the reference's playback path treats any load failure as
    end of stream, python/kspecanal.py:559-563)."""

    def __init__(self, path, sample_rate=2.4e6, center_freq=92e6, loop=False, iq_format="u8"):
        super().__init__()
        if iq_format not in IQ_FORMATS:
            raise ValueError("FileSdr: unknown iq_format [%s] (u8 | s8 | s16)" % iq_format)
        self.sample_rate, self.center_freq = sample_rate, center_freq
        self._raw = np.memmap(path, dtype=np.uint8, mode="r")
        self._pos = 0
        self.loop = loop
        self.iq_format = iq_format
        self._dtype = IQ_FORMATS[iq_format][0]
        self._bps = 2 * self._dtype.itemsize               # bytes per IQ sample

    def read_bytes(self, nbytes):
        nbytes = int(nbytes)
        if self._pos + nbytes > len(self._raw):
            if not self.loop or nbytes > len(self._raw):
                raise EOFError("capture exhausted")
            self._pos = 0
        out = np.array(self._raw[self._pos:self._pos + nbytes])
        self._pos += nbytes
        return out

    def read_iq(self, n, fmt=None):
        """n samples of the capture untouched: 2*n values of the capture format's dtype."""
        if fmt is not None and fmt != self.iq_format:
            raise ValueError("FileSdr: the capture is %s, not %s" % (self.iq_format, fmt))
        return self.read_bytes(self._bps * int(n)).view(self._dtype)

    def read_samples(self, n):
        return unpack(self.read_iq(n), self.iq_format)

    def _unpack(self, b):
        return unpack(b.view(self._dtype), self.iq_format)

    def read_blocks(self, k, length, raw, out):
        """Fill out[:k] exactly as k calls of kspecanal.sdr_read(self, length, raw) would: the same bytes consumed (reads of at
        most 2^18 samples, a short tail read rounded up to a power of two and cut back, K:343) and the same values (the
        capture's own uint8 / int8 / int16 I,Q, or complex64 through read_samples' unpack).  Returns the number of whole blocks
        read before the end of the capture."""
        k, length = int(k), int(length)
        unit = 2 ** 18                                     # kspecanal.SDR_READ_UNIT, K:311
        parts = [unit] * (length // unit) + ([length % unit] if length % unit else [])
        wants = [n if n >= unit else int(2 ** np.ceil(np.log2(n))) for n in parts]
        per = self._bps * sum(wants)                       # bytes one block consumes
        done = 0
        if per == self._bps * length and not self.loop:
            # every read is used whole: the blocks are back to back in the capture, one slice per group of blocks
            whole = min(k, (len(self._raw) - self._pos) // per)
            for g in range(0, whole, 64):
                m = min(64, whole - g)
                src = self._raw[self._pos:self._pos + m * per].reshape(m, per)
                out[g:g + m] = src.view(self._dtype) if raw else self._unpack(src)
                self._pos += m * per
            done = whole
        for i in range(done, k):                          # read by read, as sdr_read does (end of file, loop)
            try:
                col = 0
                for n, want in zip(parts, wants):
                    if raw:
                        out[i, 2 * col:2 * (col + n)] = self.read_iq(want)[:2 * n]
                    else:
                        out[i, col:col + n] = self.read_samples(want)[:n]
                    col += n
            except EOFError:
                return i
        return k


class ContiguousReader:
    """read_blocks over any source with nothing thrown away: consecutive blocks are consecutive samples of the source, whatever
    the block length.  The source is still asked only for reads the dongle allows (2^18 samples, or a power of two below that,
    K:343); what such a read delivers beyond the end of a block is kept as the start of the next one.  At the end of a capture
    the reads shrink through the allowed sizes, so that the padding of a read never costs samples the capture still holds.  One
    reader serves one run: `raw` and the buffer's dtype do not change between calls."""

    def __init__(self, sdr):
        self.sdr = sdr
        self._kept = None                                  # values read from the source and not yet handed out
        self._cap = 2 ** 18                                # kspecanal.SDR_READ_UNIT, K:311; halved when the source refuses a read
        self._exact = False                                # the source ran out once: reads are no longer rounded up
        self._done = False

    def _read(self, want, raw):
        """`want` samples as sdr_read delivers them, flat: uint8 / int8 / int16 I,Q values or complex64."""
        if raw in ("s8", "s16") and hasattr(self.sdr, "read_iq"):
            return np.asarray(self.sdr.read_iq(want, raw), dtype=IQ_FORMATS[raw][0]).reshape(-1)
        if raw is True and hasattr(self.sdr, "read_bytes"):
            return np.asarray(self.sdr.read_bytes(2 * want), dtype=np.uint8).reshape(-1)
        return np.asarray(self.sdr.read_samples(want)).astype(np.complex64).reshape(-1)

    def _fill(self, row, per, raw):
        """Fill `row` (whole samples of `per` values) from what was kept, then from the source; False when the source ran out."""
        col = 0
        if self._kept is not None:
            col = min(len(self._kept), len(row))
            row[:col] = self._kept[:col]
            self._kept = self._kept[col:] if col < len(self._kept) else None
        while col < len(row):
            n = min((len(row) - col) // per, self._cap)
            want = 1 << (n.bit_length() - 1) if self._exact else 1 << (n - 1).bit_length()
            try:
                part = self._read(want, raw)
            except EOFError:
                if want <= n:                              # fewer than `want` samples are left
                    self._cap = want // 2
                self._exact = True
                if self._cap == 0:                         # not one: what this block got stays unused
                    self._kept, self._done = np.array(row[:col]), True
                    return False
                continue
            use = min(want, n) * per
            row[col:col + use] = part[:use]
            if use < len(part):
                self._kept = np.array(part[use:])
            col += use
        return True

    def read_blocks(self, k, length, raw, out):
        """Fill out[:k] with the source's next k * length samples, in the values and dtype of kspecanal.sdr_read(sdr, length, raw).
        Returns the number of whole blocks read before the end of the source; after that every call returns 0."""
        per = 1 if out.dtype.kind == "c" else 2
        for i in range(int(k)):
            if self._done or not self._fill(out[i, :int(length) * per], per, raw):
                return i
        return int(k)
