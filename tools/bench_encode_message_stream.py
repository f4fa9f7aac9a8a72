"""A stream of unpacked single-segment messages (config-2 words) packed three
ways: python tools/bench_encode_message_stream.py [--mib 64] [--reps 10]
(--mib sizes the words as tools/bench_message_stream.py does: the packed size
at a ratio of 0.375, so the default is 170.7 MiB of words)

  stream   cpk_encode_message_stream: the boundaries found on the device
  walk     the path a caller has without it: the tables walked on the host
           over a host copy of the stream (a C loop built with gcc, a
           Python / numpy loop when there is no gcc: the label says which),
           the offset arrays uploaded, the table words squeezed out on the
           device (segments must tile d_in), then cpk_encode_messages.  The
           host copy is given: bringing a device-resident stream to the host
           for the walk is not counted in this line.
  download the device-resident stream copied to pinned host memory: what a
           caller whose stream lives on the device pays on top of `walk`
  floor    cpk_encode_messages over the same messages, true offsets given and
           the tables already squeezed out

for (a) messages of 64 KiB / 0.375 of words and (b) 1 KiB / 0.375.  Timed with
HIP events on the current stream over --reps repeats after one warm-up; the
median is printed, with the spread.  Not part of bench.py.
"""
import argparse
import ctypes
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402

LIMIT = 1 << 31

WALK_C = r"""
#include <stdint.h>
/* Serialize.read's table walk over unpacked words: segment begins and word
 * offsets, message segment offsets; returns the messages (no validation). */
uint64_t walk(const uint64_t *w, uint64_t W, uint64_t *beg, uint64_t *swo, uint64_t *mso) {
  const uint32_t *u = (const uint32_t *)w;
  uint64_t x = 0, m = 0, s = 0;
  swo[0] = 0; mso[0] = 0;
  while (x < W) {
    const uint32_t count = u[2 * x] + 1;
    uint64_t pos = x + 1 + (count & ~1u) / 2;
    for (uint32_t i = 0; i < count; ++i) {
      const uint32_t sz = u[2 * x + 1 + i];
      beg[s] = pos; swo[s + 1] = swo[s] + sz; pos += sz; ++s;
    }
    mso[++m] = s; x = pos;
  }
  return m;
}
"""


def c_walker(tmp):
    if not shutil.which("gcc"):
        return None
    src, lib = Path(tmp) / "walk.c", Path(tmp) / "walk.so"
    src.write_text(WALK_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", str(lib), str(src)], check=True)
    f = ctypes.CDLL(str(lib)).walk
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 3
    f.restype = ctypes.c_uint64
    return f


def py_walk(words, beg, swo, mso):
    u, W = words.view(np.uint32), len(words)
    x = m = s = 0
    while x < W:
        count = int(u[2 * x]) + 1
        pos = x + 1 + (count & ~1) // 2
        for sz in u[2 * x + 1: 2 * x + 1 + count]:
            beg[s] = pos
            swo[s + 1] = swo[s] + int(sz)
            pos += int(sz)
            s += 1
        m += 1
        mso[m] = s
        x = pos
    return m


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def case(ctx, label, seg_words, nm, reps, walker):
    i64 = dict(dtype=torch.int64, device="cuda")
    swo = np.arange(nm + 1, dtype=np.uint64) * seg_words
    d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
    d_mso = torch.arange(nm + 1, **i64)
    words = nm * seg_words
    d_in = torch.empty(words, **i64)
    ctx.generate(cp.preset(2), d_swo, d_in)
    # the flat unpacked stream: each message's one-word table, then its segment
    flat = words + nm
    d_flat = torch.empty(flat, **i64)
    d_flat.view(nm, seg_words + 1)[:, 0] = seg_words << 32
    d_flat.view(nm, seg_words + 1)[:, 1:] = d_in.view(nm, seg_words)
    h_flat = d_flat.cpu().numpy().view(np.uint64)  # (the host copy the walk is given)
    cap = cp.batch_capacity(swo) + 20 * nm + 64
    cap = (cap + 255) // 256 * 256
    res = {}

    # ---- the floor: true offsets given, tables squeezed out already
    d_fpk = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_foff = torch.zeros(2 * nm + 1, **i64)

    def floor():
        ctx.encode_messages(d_in, d_swo, d_mso, seg_words, d_fpk, d_foff)
    t_f = timed(floor, reps)
    P = int(d_foff[-1].item())

    # ---- the new call
    d_pk = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_off, d_mp = torch.zeros(2 * nm + 1, **i64), torch.zeros(nm + 1, **i64)

    def stream():
        res["s"] = ctx.encode_message_stream(d_flat, flat, d_pk, d_off, d_mp, LIMIT)
    t_s = timed(stream, reps)
    rc, info = res["s"]
    ok_s = (rc == 0 and info == [nm, 2 * nm, flat, P, 0, seg_words] and torch.equal(d_off, d_foff)
            and torch.equal(d_mp, 2 * d_mso) and torch.equal(d_pk[:P], d_fpk[:P]))

    # ---- today's path: host walk, upload, squeeze, cpk_encode_messages
    h_beg, h_swo, h_mso = (np.zeros(nm + 1, np.uint64) for _ in range(3))
    d_wpk = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_woff = torch.zeros(2 * nm + 1, **i64)

    def walk():
        if walker:
            m = walker(h_flat.ctypes.data, flat, h_beg.ctypes.data, h_swo.ctypes.data, h_mso.ctypes.data)
        else:
            m = py_walk(h_flat, h_beg, h_swo, h_mso)
        u_swo = torch.from_numpy(h_swo.view(np.int64)).cuda()
        u_mso = torch.from_numpy(h_mso.view(np.int64)).cuda()
        u_beg = torch.from_numpy(h_beg[:-1].view(np.int64)).cuda()
        # segment j's words flat[beg[j] : beg[j] + len[j]] -> squeezed[swo[j] : swo[j + 1]]
        lens = u_swo[1:] - u_swo[:-1]
        idx = torch.arange(int(h_swo[-1]), **i64) + torch.repeat_interleave(u_beg - u_swo[:-1], lens)
        d_sq = d_flat[idx]
        ctx.encode_messages(d_sq, u_swo, u_mso, int((h_swo[1:] - h_swo[:-1]).max()), d_wpk, d_woff)
        res["w"] = m
    t_w = timed(walk, reps)
    ok_w = res["w"] == nm and torch.equal(d_woff, d_foff) and torch.equal(d_wpk[:P], d_fpk[:P])

    # ---- what the walk needs first when the stream is device-resident
    h_pin = torch.empty(flat, dtype=torch.int64, pin_memory=True)
    t_d = timed(lambda: h_pin.copy_(d_flat, non_blocking=True), reps)

    def fmt(t):
        return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    print(f"({label}) {nm} messages of {seg_words} words, {8 * flat / (1 << 20):.1f} MiB unpacked, "
          f"{P / (1 << 20):.1f} MiB packed", flush=True)
    print(f"    stream {fmt(t_s)} ok={ok_s}  {1e3 * (t_s[0] - t_f[0]) / nm:.3f} us per message over the floor",
          flush=True)
    print(f"    walk   {fmt(t_w)} ok={ok_w}  ({'C' if walker else 'Python'} walk)", flush=True)
    print(f"    download {fmt(t_d)}", flush=True)
    print(f"    floor  {fmt(t_f)}", flush=True)
    return ok_s and ok_w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=64.0, help="packed size of the stream at a ratio of 0.375")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    ctx = cp.Context(0)
    ok = True
    try:
        with tempfile.TemporaryDirectory() as tmp:
            walker = c_walker(tmp)
            for label, kib in (("a", 64), ("b", 1)):
                seg_words = int(kib * 1024 / 8 / 0.375)
                nm = int(a.mib * 1024 / kib)
                ok &= case(ctx, label, seg_words, nm, a.reps, walker)
    finally:
        ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
