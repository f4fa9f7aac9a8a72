"""Host-side binding of the MI355X packed codec (C ABI: include/capnp_packed.h).

Mirrors capnproto-java's packed API for the hot path:
  * encode_batch / decode_batch -- n independent pieces, device-resident
    (each piece = one PackedOutputStream.write / PackedInputStream.read,
    runtime/src/main/java/org/capnproto/PackedOutputStream.java:35-205,
    PackedInputStream.java:35-140).
  * encode_messages / decode_messages -- SerializePacked.write / read per
    message (Serialize.java:256-288, :119-178), segment tables on the device.
  * host-memory forms (encode_host, decode_host, *_gather, decode_stream_host)
    for ByteBuffers that start and end in host memory.
The reference's stream classes themselves are mirrored in C++
(csrc/host/packed_stream.hpp) and Java (java/).

torch is used only for device memory and streams.  There is no CPU fallback:
if the HIP library cannot be loaded every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parents[1]
LIB_PATH = _PKG / "lib" / "libcapnp_packed_hip.so"

OK, EINVAL, ETRUNC, EOVERRUN, ETRAILING, ENOMEM, EDEVICE, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -8
EFRAME = -7  # segment table invalid (Serialize.java:45-53, :125-163)

EXPORTS = [
    "cpk_abi_version", "cpk_status_string", "cpk_packed_bound", "cpk_batch_packed_capacity",
    "cpk_ctx_create", "cpk_ctx_destroy", "cpk_ctx_device", "cpk_encode_batch",
    "cpk_decode_batch", "cpk_decode_stream", "cpk_encode_host", "cpk_decode_host",
    "cpk_decode_stream_host", "cpk_generate", "cpk_count_mismatch", "cpk_ctx_take_error",
    "cpk_decode_messages", "cpk_encode_messages", "cpk_encode_messages_host",
    "cpk_decode_messages_host", "cpk_encode_host_gather", "cpk_encode_messages_host_gather",
    "cpk_read_message", "cpk_read_message_host", "cpk_ctx_small_fallbacks",
    "cpk_encode_batch_cap", "cpk_encode_messages_cap", "cpk_ctx_dense_windows",
    "cpk_decode_message_stream", "cpk_decode_message_stream_host",
    "cpk_encode_message_stream", "cpk_encode_message_stream_host",
    "cpk_packed_size_batch", "cpk_packed_size_messages", "cpk_packed_size_host",
    "cpk_packed_size_messages_host",
    "cpk_unpacked_size_batch", "cpk_unpacked_size_host",
    "cpk_encode_batch_at",
    "cpk_decode_batch_at", "cpk_unpacked_size_batch_at",
    "cpk_decode_messages_at",
    "cpk_encode_messages_at",
]
MAT_TOTALS = 3  # CPK_MAT_TOTALS
MSG_HEAD_WORDS, MSG_INFO_WORDS = 257, 517  # CPK_MSG_HEAD_WORDS, CPK_MSG_INFO_WORDS
MS_INFO_WORDS = 5  # CPK_MS_INFO_WORDS
EMS_INFO_WORDS = 6  # CPK_EMS_INFO_WORDS


class CodecError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"{what}: {status_string(status)} ({status})" if what else status_string(status))


class DecodeException(CodecError):
    """org.capnproto.DecodeException (runtime/.../DecodeException.java:24-27)."""


class GenParams(ctypes.Structure):
    _fields_ = [("t_zero0", ctypes.c_uint64), ("t_z2n", ctypes.c_uint64),
                ("t_n2z", ctypes.c_uint64), ("t_qbyte", ctypes.c_uint64),
                ("cfg", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


_lib = None


def load(path: Path | None = None, strict: bool = True) -> ctypes.CDLL:
    """Load the HIP codec library; raises if it is missing (no fallback).
    strict=False tolerates an older build without some entry points (A/B
    timing tools only)."""
    global _lib
    if _lib is not None:
        return _lib
    # (CPK_LIB: a variant build for A/B timing and profiling tools, so that no
    # probe ever overwrites the tree's library)
    p = Path(path or os.environ.get("CPK_LIB") or LIB_PATH)
    if os.environ.get("CPK_LIB") and not path:
        strict = False  # (a variant may predate some entry points)
    if not p.exists():
        raise ImportError(f"capnp_packed: HIP library {p} not built "
                          "(run python capnproto-java_amd/build_native.py)")
    L = ctypes.CDLL(str(p))
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    sig = {
        "cpk_abi_version": ([], i32),
        "cpk_status_string": ([i32], ctypes.c_char_p),
        "cpk_packed_bound": ([u64], u64),
        "cpk_batch_packed_capacity": ([vp, u32], u64),
        "cpk_ctx_create": ([i32, ctypes.POINTER(vp)], i32),
        "cpk_ctx_destroy": ([vp], None),
        "cpk_ctx_device": ([vp], i32),
        "cpk_encode_batch": ([vp, vp, vp, u32, u64, vp, vp, vp], i32),
        "cpk_encode_batch_cap": ([vp, vp, vp, u32, u64, vp, u64, vp, vp], i32),
        "cpk_encode_messages_cap": ([vp, vp, vp, u32, vp, u32, u64, vp, u64, vp, vp], i32),
        "cpk_decode_batch": ([vp, vp, vp, vp, u32, vp, vp, vp], i32),
        "cpk_encode_host": ([vp, vp, vp, u32, vp, u64, vp], i32),
        "cpk_encode_host_gather": ([vp, vp, vp, u32, vp, u64, vp], i32),
        "cpk_decode_host": ([vp, vp, vp, vp, u32, vp, vp], i32),
        "cpk_decode_stream": ([vp, vp, u64, vp, u32, vp, vp, vp, vp], i32),
        "cpk_decode_stream_host": ([vp, vp, u64, vp, u32, vp, vp, vp], i32),
        "cpk_generate": ([vp, ctypes.POINTER(GenParams), vp, u32, vp, vp], i32),
        "cpk_count_mismatch": ([vp, vp, vp, u64, vp, vp], i32),
        "cpk_ctx_take_error": ([vp, vp], i32),
        "cpk_ctx_small_fallbacks": ([vp], u64),
        "cpk_ctx_dense_windows": ([vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)], i32),
        "cpk_decode_messages": ([vp, vp, vp, u32, u64, vp, u64, vp, vp, vp, u32, vp, vp, vp, vp], i32),
        "cpk_encode_messages": ([vp, vp, vp, u32, vp, u32, u64, vp, vp, vp], i32),
        "cpk_encode_messages_host": ([vp, vp, vp, u32, vp, u32, vp, u64, vp], i32),
        "cpk_encode_messages_host_gather": ([vp, vp, vp, u32, vp, u32, vp, u64, vp], i32),
        "cpk_decode_messages_host": ([vp, vp, vp, u32, u64, vp, u64, vp, u32, vp, vp, vp], i32),
        "cpk_read_message": ([vp, vp, u64, u64, vp, u64, vp, vp], i32),
        "cpk_read_message_host": ([vp, vp, u64, u64, vp, u64, vp], i32),
        "cpk_decode_message_stream": ([vp, vp, u64, u64, vp, u64, vp, vp, u32, vp, vp, u32, vp, vp], i32),
        "cpk_decode_message_stream_host": ([vp, vp, u64, u64, vp, u64, vp, vp, u32, vp, vp, u32, vp], i32),
        "cpk_encode_message_stream": ([vp, vp, u64, u64, vp, u64, vp, u32, vp, u32, vp, vp], i32),
        "cpk_encode_message_stream_host": ([vp, vp, u64, u64, vp, u64, vp, u32, vp, u32, vp], i32),
        "cpk_packed_size_batch": ([vp, vp, vp, u32, u64, vp, vp], i32),
        "cpk_packed_size_messages": ([vp, vp, vp, u32, vp, u32, u64, vp, vp], i32),
        "cpk_packed_size_host": ([vp, vp, vp, u32, vp], i32),
        "cpk_packed_size_messages_host": ([vp, vp, vp, u32, vp, u32, vp], i32),
        "cpk_unpacked_size_batch": ([vp, vp, vp, u32, vp, vp, vp], i32),
        "cpk_unpacked_size_host": ([vp, vp, vp, u32, vp, vp], i32),
        "cpk_encode_batch_at": ([vp, vp, vp, u32, u64, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp], i32),
        "cpk_decode_batch_at": ([vp, vp, u64, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp], i32),
        "cpk_unpacked_size_batch_at": ([vp, vp, u64, vp, vp, u32, vp, vp, vp], i32),
        "cpk_decode_messages_at": ([vp, vp, u64, vp, vp, u32, u64, vp, u64, vp, vp, vp, u32, vp, vp, vp, vp, vp], i32),
        "cpk_encode_messages_at": ([vp, vp, vp, u32, vp, u32, u64, vp, u64, vp, vp, vp, vp, vp, vp], i32),
    }
    for name, (args, res) in sig.items():
        if not strict and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def status_string(s: int) -> str:
    try:
        return load().cpk_status_string(int(s)).decode()
    except ImportError:
        return f"status {s}"


def packed_bound(words: int) -> int:
    return 8 * words + 2 * ((words + 1) // 2)


def batch_capacity(seg_word_off: np.ndarray) -> int:
    w = np.diff(np.asarray(seg_word_off, dtype=np.int64))
    return int(8 * w.sum() + 2 * ((w + 1) // 2).sum() + 16)


def _check(rc: int, what: str):
    if rc != OK:
        raise CodecError(rc, what)


class Context:
    """One HIP device + its look-back workspace (cpk_ctx_create)."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = ctypes.c_void_p()
        _check(self._lib.cpk_ctx_create(device, ctypes.byref(h)), "cpk_ctx_create")
        self.handle = h
        self.device = device
        # (the decoder choice the library read at creation: CPK_DECODER 1 / 2
        # force one decoder, anything else lets the device pick by density)
        self.decoder_forced = os.environ.get("CPK_DECODER", "") in ("1", "2")

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cpk_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- device-resident batch API (torch tensors) -----------------------
    @staticmethod
    def _stream(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def encode_batch(self, d_in, d_seg_word_off, max_seg_words: int, d_out, d_out_off,
                     stream=None):
        n = d_seg_word_off.numel() - 1
        rc = self._lib.cpk_encode_batch(self.handle, d_in.data_ptr(), d_seg_word_off.data_ptr(), n,
                                        int(max_seg_words), d_out.data_ptr(), d_out_off.data_ptr(),
                                        self._stream(stream))
        _check(rc, "cpk_encode_batch")

    def encode_batch_cap(self, d_in, d_seg_word_off, max_seg_words: int, d_out, out_cap: int,
                         d_out_off, stream=None):
        """cpk_encode_batch_cap: as encode_batch, with d_out's byte capacity;
        packed bytes past it are never stored and take_error() then returns
        CPK_ENOMEM (ArrayOutputStream.java:40-42)."""
        n = d_seg_word_off.numel() - 1
        rc = self._lib.cpk_encode_batch_cap(self.handle, d_in.data_ptr(), d_seg_word_off.data_ptr(), n,
                                            int(max_seg_words), d_out.data_ptr(), int(out_cap),
                                            d_out_off.data_ptr(), self._stream(stream))
        _check(rc, "cpk_encode_batch_cap")

    def encode_messages_cap(self, d_in, d_seg_word_off, d_msg_seg_off, max_seg_words: int, d_out,
                            out_cap: int, d_out_off, stream=None):
        """cpk_encode_messages_cap: encode_messages with d_out's byte capacity."""
        nseg = d_seg_word_off.numel() - 1
        nm = d_msg_seg_off.numel() - 1
        rc = self._lib.cpk_encode_messages_cap(self.handle, d_in.data_ptr(), d_seg_word_off.data_ptr(),
                                               nseg, d_msg_seg_off.data_ptr(), nm, int(max_seg_words),
                                               d_out.data_ptr(), int(out_cap), d_out_off.data_ptr(),
                                               self._stream(stream))
        _check(rc, "cpk_encode_messages_cap")

    def take_error(self, stream=None) -> int:
        """Synchronises `stream`; CPK_ENOMEM if an encode since the last call
        would have stored packed bytes past its out_cap (the *_cap forms),
        CPK_EINVAL if it met a piece larger than its max_seg_words hint
        (output undefined)."""
        return self._lib.cpk_ctx_take_error(self.handle, self._stream(stream))

    def dense_windows(self, stream=None) -> tuple[int, int]:
        """(windows walked serially, serial walks given back) by the block
        map's dense form in the last decode (cpk_ctx_dense_windows)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._lib.cpk_ctx_dense_windows(self.handle, self._stream(stream), ctypes.byref(a),
                                               ctypes.byref(b)), "cpk_ctx_dense_windows")
        return int(a.value), int(b.value)

    def small_fallbacks(self) -> int:
        """One-launch host calls whose completion flag was still unset after
        the stream sync that stands in past 5 ms (a lost flag); 0 in normal
        operation, late launches on a busy GPU included."""
        return int(self._lib.cpk_ctx_small_fallbacks(self.handle))

    def decode_batch(self, d_packed, d_in_off, d_seg_word_off, d_out, d_status, stream=None):
        n = d_seg_word_off.numel() - 1
        rc = self._lib.cpk_decode_batch(self.handle, d_packed.data_ptr(), d_in_off.data_ptr(),
                                        d_seg_word_off.data_ptr(), n, d_out.data_ptr(),
                                        d_status.data_ptr(), self._stream(stream))
        _check(rc, "cpk_decode_batch")

    def decode_stream(self, d_packed, avail: int, d_seg_word_off, d_out, d_in_off, d_status,
                      stream=None):
        """Serialize.read-style decode of pieces back to back from one packed
        stream of `avail` bytes (cpk_decode_stream); d_in_off[n+1] gets the
        piece boundaries found.  Synchronises `stream` once for streams of
        384 KiB and more (they are cut into blocks and decoded in parallel)."""
        n = d_seg_word_off.numel() - 1
        rc = self._lib.cpk_decode_stream(self.handle, d_packed.data_ptr(), int(avail),
                                         d_seg_word_off.data_ptr(), n, d_out.data_ptr(),
                                         d_in_off.data_ptr(), d_status.data_ptr(), self._stream(stream))
        _check(rc, "cpk_decode_stream")

    def encode_messages(self, d_in, d_seg_word_off, d_msg_seg_off, max_seg_words: int, d_out,
                        d_out_off, stream=None):
        """SerializePacked.write per message (cpk_encode_messages): the
        segment tables are built and packed on the device.  d_out_off gets
        nm + nseg + 1 piece offsets in message order."""
        nseg = d_seg_word_off.numel() - 1
        nm = d_msg_seg_off.numel() - 1
        rc = self._lib.cpk_encode_messages(self.handle, d_in.data_ptr(), d_seg_word_off.data_ptr(),
                                           nseg, d_msg_seg_off.data_ptr(), nm, int(max_seg_words),
                                           d_out.data_ptr(), d_out_off.data_ptr(),
                                           self._stream(stream))
        _check(rc, "cpk_encode_messages")

    def decode_messages(self, d_packed, d_msg_off, d_out, d_seg_word_off, d_seg_in_off,
                        d_seg_status, d_msg_seg_off, d_msg_status,
                        traversal_limit_words: int = 8 * 1024 * 1024, stream=None):
        """Serialize.read per message over a batch of packed messages with
        known byte ranges (cpk_decode_messages).  Capacities come from the
        tensors' sizes.  -> (status, total words, total segments); status
        CPK_ENOMEM (nothing decoded) if the capacities are too small."""
        nm = d_msg_off.numel() - 1
        tot = (ctypes.c_uint64 * 2)()
        seg_cap = min(d_seg_status.numel() if d_seg_status is not None else 0,
                      d_seg_word_off.numel() - 1 if d_seg_word_off is not None else 0)

        def ptr(t):
            return t.data_ptr() if t is not None else None
        rc = self._lib.cpk_decode_messages(
            self.handle, d_packed.data_ptr(), d_msg_off.data_ptr(), nm, int(traversal_limit_words),
            ptr(d_out), d_out.numel() * d_out.element_size() // 8 if d_out is not None else 0,
            ptr(d_seg_word_off), ptr(d_seg_in_off), ptr(d_seg_status), seg_cap,
            d_msg_seg_off.data_ptr(), d_msg_status.data_ptr(), tot, self._stream(stream))
        if rc not in (OK, ENOMEM):
            _check(rc, "cpk_decode_messages")
        return rc, int(tot[0]), int(tot[1])

    def generate(self, params: GenParams, d_seg_word_off, d_out, stream=None):
        n = d_seg_word_off.numel() - 1
        _check(self._lib.cpk_generate(self.handle, ctypes.byref(params), d_seg_word_off.data_ptr(),
                                      n, d_out.data_ptr(), self._stream(stream)), "cpk_generate")

    def count_mismatch(self, d_a, d_b, words: int, d_cnt, stream=None):
        _check(self._lib.cpk_count_mismatch(self.handle, d_a.data_ptr(), d_b.data_ptr(), int(words),
                                            d_cnt.data_ptr(), self._stream(stream)),
               "cpk_count_mismatch")

    # ---- host-memory forms (numpy) -----------------------------------------
    def encode_host(self, data: np.ndarray, seg_word_off: np.ndarray, out: np.ndarray = None):
        """-> (packed bytes as uint8 array, out_off uint64[n+1]).  `out`: a
        reusable uint8 buffer of at least batch_capacity() bytes."""
        swo = np.ascontiguousarray(seg_word_off, dtype=np.uint64)
        n = len(swo) - 1
        data = np.ascontiguousarray(data, dtype=np.uint8)
        cap = batch_capacity(swo)
        if out is None:
            out = np.zeros(cap, dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < cap:
            raise ValueError("out: contiguous uint8, at least batch_capacity() bytes")
        off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.cpk_encode_host(self.handle, data.ctypes.data if data.size else None,
                                       swo.ctypes.data, n, out.ctypes.data, cap, off.ctypes.data)
        _check(rc, "cpk_encode_host")
        return out[: int(off[-1])], off

    def encode_host_gather(self, pieces, out: np.ndarray = None):
        """Gather form: `pieces` = list of uint64 word arrays, one per piece,
        each left where it lies (no concatenation).  -> (packed uint8, out_off)."""
        pieces = [np.ascontiguousarray(x, dtype=np.uint64) for x in pieces]
        n = len(pieces)
        swo = np.zeros(n + 1, dtype=np.uint64)
        swo[1:] = np.cumsum([x.size for x in pieces])
        ptrs = (ctypes.c_void_p * max(n, 1))(*[x.ctypes.data if x.size else None for x in pieces])
        cap = batch_capacity(swo)
        if out is None:
            out = np.zeros(cap, dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < cap:
            raise ValueError("out: contiguous uint8, at least batch_capacity() bytes")
        off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.cpk_encode_host_gather(self.handle, ptrs, swo.ctypes.data, n,
                                              out.ctypes.data, cap, off.ctypes.data)
        _check(rc, "cpk_encode_host_gather")
        return out[: int(off[-1])], off

    def decode_host(self, packed: np.ndarray, in_off: np.ndarray, seg_word_off: np.ndarray,
                    out: np.ndarray = None):
        """-> (decoded uint8 array, status int32[n]).  Never raises on bad data.
        `out`: a reusable uint8 buffer of at least 8 * seg_word_off[-1] bytes."""
        swo = np.ascontiguousarray(seg_word_off, dtype=np.uint64)
        io = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(swo) - 1
        pk = np.ascontiguousarray(packed, dtype=np.uint8)
        if out is None:
            out = np.zeros(int(8 * swo[-1]) + 8, dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < int(8 * swo[-1]):
            raise ValueError("out: contiguous uint8, at least 8 * seg_word_off[-1] bytes")
        st = np.zeros(max(n, 1), dtype=np.int32)
        rc = self._lib.cpk_decode_host(self.handle, pk.ctypes.data if pk.size else None,
                                       io.ctypes.data, swo.ctypes.data, n, out.ctypes.data,
                                       st.ctypes.data)
        if rc not in (OK, ETRUNC, EOVERRUN, ETRAILING, EUNSUPPORTED, EINVAL):
            _check(rc, "cpk_decode_host")
        return out[: int(8 * swo[-1])], st[:n]


def _encode_messages_host(self, messages):
    """SerializePacked.write for each message (a list of segments, bytes of
    whole words) -> the packed bytes of all messages, back to back."""
    segs = [bytes(s) for m in messages for s in m]
    swo = np.concatenate([[0], np.cumsum([len(s) // 8 for s in segs], dtype=np.uint64)]).astype(np.uint64)
    mso = np.concatenate([[0], np.cumsum([len(m) for m in messages], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(b"".join(segs) + b"\0" * 8, np.uint8)
    cap = batch_capacity(swo) + sum(10 * ((len(m) + 2) // 2 + 1) for m in messages)
    out = np.zeros(cap, np.uint8)
    off = np.zeros(len(messages) + len(segs) + 1, np.uint64)
    _check(self._lib.cpk_encode_messages_host(self.handle, data.ctypes.data, swo.ctypes.data,
                                              len(segs), mso.ctypes.data, len(messages),
                                              out.ctypes.data, cap, off.ctypes.data),
           "cpk_encode_messages_host")
    return out[: int(off[-1])].tobytes(), off


def _encode_messages_host_gather(self, messages):
    """As _encode_messages_host, each segment passed where it lies
    (cpk_encode_messages_host_gather)."""
    segs = [np.frombuffer(bytes(s), np.uint8) for m in messages for s in m]
    swo = np.concatenate([[0], np.cumsum([s.size // 8 for s in segs], dtype=np.uint64)]).astype(np.uint64)
    mso = np.concatenate([[0], np.cumsum([len(m) for m in messages], dtype=np.uint64)]).astype(np.uint64)
    ptrs = (ctypes.c_void_p * max(len(segs), 1))(*[s.ctypes.data if s.size else None for s in segs])
    cap = batch_capacity(swo) + sum(10 * ((len(m) + 2) // 2 + 1) for m in messages)
    out = np.zeros(cap, np.uint8)
    off = np.zeros(len(messages) + len(segs) + 1, np.uint64)
    _check(self._lib.cpk_encode_messages_host_gather(self.handle, ptrs, swo.ctypes.data,
                                                     len(segs), mso.ctypes.data, len(messages),
                                                     out.ctypes.data, cap, off.ctypes.data),
           "cpk_encode_messages_host_gather")
    return out[: int(off[-1])].tobytes(), off


def _decode_messages_host(self, packed, msg_off, traversal_limit_words: int = 8 * 1024 * 1024):
    """Serialize.read per message -> (message statuses, [[segment bytes]])."""
    pk = np.frombuffer(bytes(packed), np.uint8)
    mo = np.ascontiguousarray(msg_off, dtype=np.uint64)
    nm = len(mo) - 1
    mso = np.zeros(nm + 1, np.uint64)
    mst = np.zeros(max(nm, 1), np.int32)
    tot = np.zeros(2, np.uint64)
    pkp = pk.ctypes.data if pk.size else None
    rc = self._lib.cpk_decode_messages_host(self.handle, pkp, mo.ctypes.data, nm,
                                            traversal_limit_words, None, 0, None, 0,
                                            mso.ctypes.data, mst.ctypes.data, tot.ctypes.data)
    if rc == ENOMEM:
        out = np.zeros(int(tot[0]) * 8 + 8, np.uint8)
        sw = np.zeros(int(tot[1]) + 1, np.uint64)
        rc = self._lib.cpk_decode_messages_host(self.handle, pkp, mo.ctypes.data, nm,
                                                traversal_limit_words, out.ctypes.data, int(tot[0]),
                                                sw.ctypes.data, int(tot[1]), mso.ctypes.data,
                                                mst.ctypes.data, tot.ctypes.data)
    else:
        out, sw = np.zeros(8, np.uint8), np.zeros(1, np.uint64)
    if rc in (ENOMEM, EDEVICE):
        _check(rc, "cpk_decode_messages_host")
    msgs = [[out[8 * int(sw[j]): 8 * int(sw[j + 1])].tobytes() for j in range(int(mso[m]), int(mso[m + 1]))]
            for m in range(nm)]
    return mst[:nm], msgs


Context.encode_messages_host = _encode_messages_host
Context.encode_messages_host_gather = _encode_messages_host_gather
Context.decode_messages_host = _decode_messages_host


def _decode_stream_host(self, packed: np.ndarray, seg_word_off: np.ndarray, out: np.ndarray = None):
    """PackedInputStream.read per piece, back to back over one stream.
    -> (decoded uint8 array, piece boundaries uint64[n+1], status int32[n]).
    `out`: a reusable uint8 buffer of at least 8 * seg_word_off[-1] bytes."""
    swo = np.ascontiguousarray(seg_word_off, dtype=np.uint64)
    n = len(swo) - 1
    pk = np.ascontiguousarray(packed, dtype=np.uint8)
    if out is None:
        out = np.zeros(int(8 * swo[-1]) + 8, dtype=np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < int(8 * swo[-1]):
        raise ValueError("out: contiguous uint8, at least 8 * seg_word_off[-1] bytes")
    io = np.zeros(n + 1, dtype=np.uint64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    rc = self._lib.cpk_decode_stream_host(self.handle, pk.ctypes.data if pk.size else None,
                                          pk.size, swo.ctypes.data, n, out.ctypes.data,
                                          io.ctypes.data, st.ctypes.data)
    if rc not in (OK, ETRUNC, EOVERRUN, ETRAILING, EUNSUPPORTED, EINVAL):
        _check(rc, "cpk_decode_stream_host")
    return out[: int(8 * swo[-1])], io, st[:n]


Context.decode_stream_host = _decode_stream_host


def _read_message(self, d_packed, avail: int, d_out, d_info, traversal_limit_words: int = 8 * 1024 * 1024,
                  stream=None):
    """cpk_read_message: one message from the front of a device-resident
    packed stream (Serialize.read, Serialize.java:119-178), no host sync.
    d_out: int64 tensor of out_cap_words + MSG_HEAD_WORDS words; d_info:
    int64[MSG_INFO_WORDS], written on the device."""
    cap = d_out.numel() * d_out.element_size() // 8 - MSG_HEAD_WORDS
    if cap < 0 or d_info.numel() * d_info.element_size() < 8 * MSG_INFO_WORDS:
        raise ValueError("d_out / d_info too small")
    _check(self._lib.cpk_read_message(self.handle, d_packed.data_ptr(), int(avail), int(traversal_limit_words),
                                      d_out.data_ptr(), cap, d_info.data_ptr(), self._stream(stream)),
           "cpk_read_message")


def _read_message_host(self, packed, out_cap_words: int | None = None,
                       traversal_limit_words: int = 8 * 1024 * 1024):
    """cpk_read_message_host -> (status, [segment bytes], bytes consumed,
    info row).  out_cap_words None: sized by a first call (CPK_ENOMEM gives
    the words needed)."""
    pk = np.ascontiguousarray(np.frombuffer(bytes(packed), np.uint8) if not isinstance(packed, np.ndarray)
                              else packed, dtype=np.uint8)
    info = np.zeros(MSG_INFO_WORDS, np.uint64)
    cap = 0 if out_cap_words is None else int(out_cap_words)
    for _ in range(2):
        out = np.zeros(max(cap, 1), np.uint64)
        rc = self._lib.cpk_read_message_host(self.handle, pk.ctypes.data if pk.size else None, pk.size,
                                             int(traversal_limit_words), out.ctypes.data, cap,
                                             info.ctypes.data)
        if rc == ENOMEM and out_cap_words is None and int(info[3]) > cap:
            cap = int(info[3])
            continue
        break
    if rc in (EDEVICE, EINVAL) or (rc == ENOMEM and int(info.view(np.int64)[0]) != ENOMEM):
        _check(rc, "cpk_read_message_host")
    if rc != OK:
        return rc, [], 0, info
    n = int(info[2])
    b = out.view(np.uint8)
    segs = [b[8 * int(info[4 + i]): 8 * int(info[5 + i])].tobytes() for i in range(n)]
    return rc, segs, int(info[1]), info


Context.read_message = _read_message
Context.read_message_host = _read_message_host


def _decode_message_stream(self, d_packed, avail: int, d_out, d_msg_off, d_msg_seg_off, d_seg_begin,
                           d_seg_words, traversal_limit_words: int = 8 * 1024 * 1024, stream=None):
    """cpk_decode_message_stream: a loop of SerializePacked.read over a
    device-resident stream of packed messages whose boundaries are not known.
    d_out gets the flat unpacked stream; segment j is d_out[d_seg_begin[j] :
    + d_seg_words[j]].  Capacities come from the tensors' sizes (None: 0).
    -> (rc, info): rc CPK_OK or CPK_ENOMEM (info then holds the sizes
    needed); info = [messages, segments, words, bytes consumed, tail status]."""
    def ptr(t):
        return t.data_ptr() if t is not None else None

    def words(t):
        return t.numel() * t.element_size() // 8 if t is not None else 0
    msg_cap = max(min(words(d_msg_off), words(d_msg_seg_off)) - 1, 0)
    seg_cap = min(words(d_seg_begin), words(d_seg_words))
    if words(d_msg_off) == 0 or words(d_msg_seg_off) == 0:
        d_msg_off = d_msg_seg_off = None
    info = np.zeros(MS_INFO_WORDS, np.uint64)
    rc = self._lib.cpk_decode_message_stream(
        self.handle, d_packed.data_ptr(), int(avail), int(traversal_limit_words), ptr(d_out), words(d_out),
        ptr(d_msg_off), ptr(d_msg_seg_off), msg_cap, ptr(d_seg_begin), ptr(d_seg_words), seg_cap,
        info.ctypes.data, self._stream(stream))
    if rc not in (OK, ENOMEM):
        _check(rc, "cpk_decode_message_stream")
    out = [int(v) for v in info]
    out[4] = int(info.view(np.int64)[4])
    return rc, out


def _decode_message_stream_host(self, packed, traversal_limit_words: int = 8 * 1024 * 1024):
    """cpk_decode_message_stream_host -> (tail status, [[segment bytes]],
    bytes consumed): every complete message of the stream, in order.  Sized
    by the CPK_ENOMEM protocol: the words first, then the arrays."""
    pk = np.ascontiguousarray(np.frombuffer(bytes(packed), np.uint8) if not isinstance(packed, np.ndarray)
                              else packed, dtype=np.uint8)
    info = np.zeros(MS_INFO_WORDS, np.uint64)
    words = nm = ns = 0
    for _ in range(3):
        out = np.zeros(max(words, 1), np.uint64)
        mo, mso = np.zeros(nm + 1, np.uint64), np.zeros(nm + 1, np.uint64)
        sb, sw = np.zeros(max(ns, 1), np.uint64), np.zeros(max(ns, 1), np.uint64)
        rc = self._lib.cpk_decode_message_stream_host(
            self.handle, pk.ctypes.data if pk.size else None, pk.size, int(traversal_limit_words),
            out.ctypes.data, words, mo.ctypes.data, mso.ctypes.data, nm, sb.ctypes.data, sw.ctypes.data, ns,
            info.ctypes.data)
        if rc != ENOMEM:
            break
        words, nm, ns = max(words, int(info[2])), max(nm, int(info[0])), max(ns, int(info[1]))
    _check(rc, "cpk_decode_message_stream_host")
    b = out.view(np.uint8)
    msgs = [[b[8 * int(sb[j]): 8 * int(sb[j] + sw[j])].tobytes() for j in range(int(mso[m]), int(mso[m + 1]))]
            for m in range(int(info[0]))]
    return int(info.view(np.int64)[4]), msgs, int(info[3])


Context.decode_message_stream = _decode_message_stream
Context.decode_message_stream_host = _decode_message_stream_host


def _encode_message_stream(self, d_in, avail_words: int, d_out, d_out_off, d_msg_piece,
                           traversal_limit_words: int = 8 * 1024 * 1024, stream=None):
    """cpk_encode_message_stream: a loop of Serialize.read over a
    device-resident stream of unpacked messages whose boundaries are not known
    (what decode_message_stream writes), each message packed as
    SerializePacked.write packs it.  d_out gets the packed bytes, d_out_off the
    piece offsets (table, segments; next message), d_msg_piece each message's
    first piece.  Capacities come from the tensors' sizes (None: 0).
    -> (rc, info): rc CPK_OK or CPK_ENOMEM (info then holds the sizes needed);
    info = [messages, pieces, words consumed, packed bytes, tail status,
    largest piece in words]."""
    def ptr(t):
        return t.data_ptr() if t is not None else None

    def words(t):
        return t.numel() * t.element_size() // 8 if t is not None else 0
    if words(d_out_off) == 0:
        d_out_off = None
    if words(d_msg_piece) == 0:
        d_msg_piece = None
    out_cap = d_out.numel() * d_out.element_size() if d_out is not None else 0
    info = np.zeros(EMS_INFO_WORDS, np.uint64)
    rc = self._lib.cpk_encode_message_stream(
        self.handle, ptr(d_in), int(avail_words), int(traversal_limit_words), ptr(d_out) if out_cap else None,
        out_cap, ptr(d_out_off), max(words(d_out_off) - 1, 0), ptr(d_msg_piece), max(words(d_msg_piece) - 1, 0),
        info.ctypes.data, self._stream(stream))
    if rc not in (OK, ENOMEM):
        _check(rc, "cpk_encode_message_stream")
    out = [int(v) for v in info]
    out[4] = int(info.view(np.int64)[4])
    return rc, out


def _encode_message_stream_host(self, words_or_bytes, traversal_limit_words: int = 8 * 1024 * 1024):
    """cpk_encode_message_stream_host -> (tail status, packed bytes, out_off
    uint64[pieces + 1], msg_piece uint64[messages + 1], words consumed): every
    complete message of the unpacked stream, packed in order.  Whole words
    only (trailing bytes short of a word are not part of the stream).  Sized
    by the CPK_ENOMEM protocol: the arrays first, then the bytes."""
    if isinstance(words_or_bytes, np.ndarray):
        w = np.ascontiguousarray(words_or_bytes).view(np.uint8).reshape(-1)
    else:
        w = np.frombuffer(bytes(words_or_bytes), np.uint8)
    nw = w.size // 8
    w = np.ascontiguousarray(w[: 8 * nw]).view(np.uint64) if nw else np.zeros(1, np.uint64)
    info = np.zeros(EMS_INFO_WORDS, np.uint64)
    cap = np_ = nm = 0
    for _ in range(3):
        out = np.zeros(max(cap, 1), np.uint8)
        off, mp = np.zeros(np_ + 1, np.uint64), np.zeros(nm + 1, np.uint64)
        rc = self._lib.cpk_encode_message_stream_host(
            self.handle, w.ctypes.data if nw else None, nw, int(traversal_limit_words),
            out.ctypes.data if cap else None, cap, off.ctypes.data, np_, mp.ctypes.data, nm, info.ctypes.data)
        if rc != ENOMEM:
            break
        cap, np_, nm = max(cap, int(info[3])), max(np_, int(info[1])), max(nm, int(info[0]))
    _check(rc, "cpk_encode_message_stream_host")
    return (int(info.view(np.int64)[4]), out[: int(info[3])].tobytes(), off[: int(info[1]) + 1],
            mp[: int(info[0]) + 1], int(info[2]))


Context.encode_message_stream = _encode_message_stream
Context.encode_message_stream_host = _encode_message_stream_host


def _packed_size_batch(self, d_in, d_seg_word_off, max_seg_words: int, d_out_off, stream=None):
    """cpk_packed_size_batch: d_out_off[n+1] gets exactly what encode_batch
    would write there for the same arguments -- no packed byte is produced,
    no output buffer taken; d_out_off[n] is the total.  max_seg_words = 0
    synchronises `stream` once, as encode_batch does."""
    n = d_seg_word_off.numel() - 1
    rc = self._lib.cpk_packed_size_batch(self.handle, d_in.data_ptr(), d_seg_word_off.data_ptr(), n,
                                         int(max_seg_words), d_out_off.data_ptr(), self._stream(stream))
    _check(rc, "cpk_packed_size_batch")


def _packed_size_messages(self, d_in, d_seg_word_off, d_msg_seg_off, max_seg_words: int, d_out_off,
                          stream=None):
    """cpk_packed_size_messages: d_out_off[nm + nseg + 1] as encode_messages
    lays it out (per message the table piece, then its segments)."""
    nseg = d_seg_word_off.numel() - 1
    nm = d_msg_seg_off.numel() - 1
    rc = self._lib.cpk_packed_size_messages(self.handle, d_in.data_ptr(), d_seg_word_off.data_ptr(), nseg,
                                            d_msg_seg_off.data_ptr(), nm, int(max_seg_words),
                                            d_out_off.data_ptr(), self._stream(stream))
    _check(rc, "cpk_packed_size_messages")


def _packed_size_host(self, data: np.ndarray, seg_word_off: np.ndarray) -> np.ndarray:
    """cpk_packed_size_host -> out_off uint64[n+1]: the packed piece offsets
    encode_host would return, without the packed bytes."""
    swo = np.ascontiguousarray(seg_word_off, dtype=np.uint64)
    n = len(swo) - 1
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    off = np.zeros(n + 1, dtype=np.uint64)
    _check(self._lib.cpk_packed_size_host(self.handle, data.ctypes.data if data.size else None,
                                          swo.ctypes.data, n, off.ctypes.data), "cpk_packed_size_host")
    return off


def _packed_size_messages_host(self, messages) -> np.ndarray:
    """cpk_packed_size_messages_host for a list of messages (each a list of
    segments, bytes of whole words) -> out_off uint64[messages + segments +
    1] in message order (table, segments); the last entry is the length of
    what SerializePacked.write would produce for all of them."""
    segs = [bytes(s) for m in messages for s in m]
    swo = np.concatenate([[0], np.cumsum([len(s) // 8 for s in segs], dtype=np.uint64)]).astype(np.uint64)
    mso = np.concatenate([[0], np.cumsum([len(m) for m in messages], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(b"".join(segs) + b"\0" * 8, np.uint8)
    off = np.zeros(len(messages) + len(segs) + 1, np.uint64)
    _check(self._lib.cpk_packed_size_messages_host(self.handle, data.ctypes.data, swo.ctypes.data, len(segs),
                                                   mso.ctypes.data, len(messages), off.ctypes.data),
           "cpk_packed_size_messages_host")
    return off


def _unpacked_size_batch(self, d_packed, d_in_off, d_seg_word_off, d_status, stream=None):
    """cpk_unpacked_size_batch: d_seg_word_off[n+1] gets the word offsets
    decode_batch must be given for the packed ranges d_in_off[n+1] -- no word
    is decoded; d_seg_word_off[n] is the total.  d_status[n]: OK, or ETRUNC
    for a range that ends inside a record (it sizes to 0 words).  A batch of
    at most 32 pieces synchronises `stream` once, as decode_batch does."""
    n = d_in_off.numel() - 1
    rc = self._lib.cpk_unpacked_size_batch(self.handle, d_packed.data_ptr(), d_in_off.data_ptr(), n,
                                           d_seg_word_off.data_ptr(), d_status.data_ptr() if n else None,
                                           self._stream(stream))
    _check(rc, "cpk_unpacked_size_batch")


def _unpacked_size_host(self, packed: np.ndarray, in_off: np.ndarray):
    """cpk_unpacked_size_host -> (seg_word_off uint64[n+1], status int32[n]):
    what decode_host needs besides the packed ranges.  Never raises on bad
    data: a truncated piece has status ETRUNC and 0 words."""
    io = np.ascontiguousarray(in_off, dtype=np.uint64)
    n = len(io) - 1
    pk = np.ascontiguousarray(packed, dtype=np.uint8)
    swo = np.zeros(n + 1, dtype=np.uint64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    rc = self._lib.cpk_unpacked_size_host(self.handle, pk.ctypes.data if pk.size else None, io.ctypes.data, n,
                                          swo.ctypes.data, st.ctypes.data)
    if rc not in (OK, ETRUNC):
        _check(rc, "cpk_unpacked_size_host")
    return swo, st[:n]


def _encode_batch_at(self, d_in, d_seg_word_off, max_seg_words: int, d_grp_piece_off, d_out, out_cap: int,
                     d_dst_off, d_dst_cap, d_piece_off, d_grp_len, d_status, stream=None, ng=None):
    """cpk_encode_batch_at: the pieces packed to where the caller says.  Group
    g (pieces d_grp_piece_off[g] .. [g+1]; None: every piece its own group)
    goes to d_out + d_dst_off[g], into a slot of d_dst_cap[g] bytes (None: to
    out_cap -- d_dst_off may then be packed_size_batch's output as it stands).
    Written: d_piece_off[n], d_grp_len[ng], d_status[ng] (OK, ENOMEM for a slot
    too small or past out_cap, EINVAL for a piece over max_seg_words); no byte
    of d_out outside the groups' packed bytes is touched.  ng: the group count
    when it is not d_grp_piece_off's (or, without groups, the piece count)."""
    ptr = lambda t: t.data_ptr() if t is not None else None
    n = d_seg_word_off.numel() - 1
    if ng is None:
        ng = d_grp_piece_off.numel() - 1 if d_grp_piece_off is not None else n
    rc = self._lib.cpk_encode_batch_at(self.handle, ptr(d_in), d_seg_word_off.data_ptr(), n, int(max_seg_words),
                                       ptr(d_grp_piece_off), int(ng), ptr(d_out), int(out_cap), ptr(d_dst_off),
                                       ptr(d_dst_cap), ptr(d_piece_off), ptr(d_grp_len), ptr(d_status),
                                       self._stream(stream))
    _check(rc, "cpk_encode_batch_at")


def _decode_batch_at(self, d_packed, in_cap: int, d_src_off, d_src_len, d_grp_piece_off, d_seg_word_off, d_out,
                     d_status, d_grp_status, d_grp_used, stream=None, ng=None):
    """cpk_decode_batch_at: the pieces decoded from where the caller says.
    Group g (pieces d_grp_piece_off[g] .. [g+1], read back to back; None: every
    piece its own group) is the packed bytes d_packed[d_src_off[g] ..
    d_src_off[g] + d_src_len[g]), any alignment, order and gaps, below in_cap.
    Piece i goes to words d_seg_word_off[i] .. [i+1] of d_out.  Written:
    d_status[n], d_grp_status[ng] (OK, the first failed piece's status,
    ETRAILING, EINVAL for a range past in_cap, EUNSUPPORTED for one over 2^32-1
    bytes), d_grp_used[ng].  The arrays of an encode_batch_at call decode what
    it wrote: d_dst_off as d_src_off, d_grp_len as d_src_len.  ng: the group
    count when it is not d_grp_piece_off's (or, without groups, the piece
    count)."""
    ptr = lambda t: t.data_ptr() if t is not None else None
    n = d_seg_word_off.numel() - 1 if d_seg_word_off is not None else 0
    if ng is None:
        ng = d_grp_piece_off.numel() - 1 if d_grp_piece_off is not None else n
    rc = self._lib.cpk_decode_batch_at(self.handle, ptr(d_packed), int(in_cap), ptr(d_src_off), ptr(d_src_len),
                                       ptr(d_grp_piece_off), int(ng), ptr(d_seg_word_off), n, ptr(d_out),
                                       ptr(d_status), ptr(d_grp_status), ptr(d_grp_used), self._stream(stream))
    _check(rc, "cpk_decode_batch_at")


def _unpacked_size_batch_at(self, d_packed, in_cap: int, d_src_off, d_src_len, d_seg_word_off, d_status,
                            stream=None):
    """cpk_unpacked_size_batch_at: unpacked_size_batch over the ranges
    d_packed[d_src_off[i] .. d_src_off[i] + d_src_len[i]): d_seg_word_off[n+1]
    gets the word offsets decode_batch_at must be given, d_status[n] OK, ETRUNC,
    or a refused range's EINVAL / EUNSUPPORTED (each sized 0).  Never
    synchronises."""
    ptr = lambda t: t.data_ptr() if t is not None else None
    n = d_seg_word_off.numel() - 1
    rc = self._lib.cpk_unpacked_size_batch_at(self.handle, ptr(d_packed), int(in_cap), ptr(d_src_off),
                                              ptr(d_src_len), n, d_seg_word_off.data_ptr(), ptr(d_status),
                                              self._stream(stream))
    _check(rc, "cpk_unpacked_size_batch_at")


def _decode_messages_at(self, d_packed, in_cap: int, d_src_off, d_src_len, d_out, d_seg_word_off, d_seg_in_off,
                        d_seg_status, d_msg_seg_off, d_msg_status, d_msg_used, d_totals,
                        traversal_limit_words: int = 8 * 1024 * 1024, stream=None, nm=None, out_cap_words=None,
                        seg_cap=None):
    """cpk_decode_messages_at: Serialize.read per message over the packed bytes
    d_packed[d_src_off[m] .. d_src_off[m] + d_src_len[m]), any alignment, order
    and gaps, below in_cap; the tables are read on the device and nothing comes
    back to the host.  Capacities come from the tensors' sizes unless given;
    d_out and the three segment arrays may be None (a sizing call).  Written:
    d_msg_seg_off[nm+1], d_msg_status[nm] (OK, ETRAILING, a range's EINVAL /
    EUNSUPPORTED, the table's or a segment's error, ENOMEM for an accepted
    message past the capacities), d_msg_used[nm], d_totals[3] (the accepted
    messages' words and segments, the messages that fit) and, for the fitting
    messages, the words and the segment arrays as decode_messages tiles them.
    Never synchronises."""
    ptr = lambda t: t.data_ptr() if t is not None else None
    if nm is None:
        nm = d_msg_seg_off.numel() - 1
    if out_cap_words is None:
        out_cap_words = d_out.numel() * d_out.element_size() // 8 if d_out is not None else 0
    if seg_cap is None:
        seg_cap = 0 if d_seg_word_off is None or d_seg_in_off is None or d_seg_status is None else \
            min(d_seg_word_off.numel() - 1, d_seg_in_off.numel(), d_seg_status.numel())
    rc = self._lib.cpk_decode_messages_at(self.handle, ptr(d_packed), int(in_cap), ptr(d_src_off), ptr(d_src_len),
                                          int(nm), int(traversal_limit_words), ptr(d_out), int(out_cap_words),
                                          ptr(d_seg_word_off), ptr(d_seg_in_off), ptr(d_seg_status), int(seg_cap),
                                          ptr(d_msg_seg_off), ptr(d_msg_status), ptr(d_msg_used), ptr(d_totals),
                                          self._stream(stream))
    _check(rc, "cpk_decode_messages_at")


def _encode_messages_at(self, d_in, d_seg_word_off, d_msg_seg_off, max_seg_words: int, d_out, out_cap: int,
                        d_dst_off, d_dst_cap, d_piece_off, d_msg_len, d_status, stream=None, nm=None, nseg=None):
    """cpk_encode_messages_at: SerializePacked.write of message m (segments
    d_msg_seg_off[m] .. [m+1], its table built on the device) to d_out +
    d_dst_off[m], into a slot of d_dst_cap[m] bytes (None: to out_cap).
    max_seg_words is required.  Written: d_piece_off[nm + nseg] (message order:
    table, segments), d_msg_len[nm], d_status[nm] (OK, ENOMEM for a slot too
    small or past out_cap, EINVAL for a segment over max_seg_words); no byte of
    d_out outside the messages' packed bytes is touched.  d_dst_off / d_msg_len
    are decode_messages_at's d_src_off / d_src_len.  Never synchronises.  nm,
    nseg: the counts when they are not the offset arrays'."""
    ptr = lambda t: t.data_ptr() if t is not None else None
    if nseg is None:
        nseg = d_seg_word_off.numel() - 1 if d_seg_word_off is not None else 0
    if nm is None:
        nm = d_msg_seg_off.numel() - 1 if d_msg_seg_off is not None else 0
    rc = self._lib.cpk_encode_messages_at(self.handle, ptr(d_in), ptr(d_seg_word_off), int(nseg),
                                          ptr(d_msg_seg_off), int(nm), int(max_seg_words), ptr(d_out), int(out_cap),
                                          ptr(d_dst_off), ptr(d_dst_cap), ptr(d_piece_off), ptr(d_msg_len),
                                          ptr(d_status), self._stream(stream))
    _check(rc, "cpk_encode_messages_at")


Context.encode_batch_at = _encode_batch_at
Context.encode_messages_at = _encode_messages_at
Context.decode_batch_at = _decode_batch_at
Context.decode_messages_at = _decode_messages_at
Context.unpacked_size_batch_at = _unpacked_size_batch_at
Context.packed_size_batch = _packed_size_batch
Context.unpacked_size_batch = _unpacked_size_batch
Context.unpacked_size_host = _unpacked_size_host
Context.packed_size_messages = _packed_size_messages
Context.packed_size_host = _packed_size_host
Context.packed_size_messages_host = _packed_size_messages_host


def gen_params(cfg: int, z: float, lz: float, q: float) -> GenParams:
    """Thresholds of the synthetic 2-state Markov generator, out of 2^31:
    `FastRand.nextInt()` never returns a negative value (Common.java:31-38,
    arithmetic `>>` clears bit 31), so a draw lies in [0, 2^31)."""
    def thr(p):
        return int(min(max(p, 0.0), 1.0) * (1 << 31))
    a = 1.0 / lz
    b = 1.0 if z >= 1.0 else a * z / (1.0 - z)
    return GenParams(thr(z), thr(a), thr(b), thr(q), cfg, 0)


CONFIGS = {
    2: dict(z=0.5, lz=4.0, q=0.25),
    3: dict(z=0.05, lz=1.5, q=1 / 256),
    4: dict(z=0.9, lz=64.0, q=0.25),
}


def preset(cfg: int) -> GenParams:
    c = CONFIGS[cfg]
    return gen_params(cfg, c["z"], c["lz"], c["q"])
