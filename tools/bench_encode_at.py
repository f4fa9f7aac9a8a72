"""Size + placed encode against the encode that places for itself, device-resident:
python tools/bench_encode_at.py [--rows p2,p3,p4,dominant,tiny] [--reps 10] [--parent-lib PATH]

Rows (each generated on the device, cpk_generate):
  p2 p3 p4   131,072 pieces of 8192 words at presets 2, 3 and 4
  dominant   one piece of 8 Mi words beside 1,024 of 2048 (preset 2)
  tiny       1 Mi pieces of 64 words (preset 2): a workgroup per piece
Columns, HIP events on the current stream, the median of --reps repeats after
one warm-up, with the spread:
  encode     cpk_encode_batch.  With --parent-lib (another build of the
             library, e.g. the parent commit's) the call goes to that library
             through a context of its own, on the same batch in this process;
             without it to the tree's library, and the line says so.
  size       cpk_packed_size_batch
  at         cpk_encode_batch_at, d_dst_off = the size call's offsets as they
             stand, d_dst_cap = NULL, out_cap = the exact total
  size+at    the sum of the two medians
  at+16      the same with a 16-byte gap in front of every piece (a length
             prefix's room): d_dst_off[i] = offset[i] + 16 (i + 1)
The placed bytes are compared with cpk_encode_batch's in the same run
(mismatch = differing bytes of the packed stream, 0 expected); for the gapped
layout the statuses, lengths and piece offsets are.  CPK_AT_FORM=dense|sparse
forces the placed kernel's form.  Not part of bench.py.
"""
import argparse
import ctypes
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402

ROWS = {
    "p2": (2, [(131072, 8192)]),
    "p3": (3, [(131072, 8192)]),
    "p4": (4, [(131072, 8192)]),
    "dominant": (2, [(1, 8 << 20), (1024, 2048)]),
    "tiny": (2, [(1 << 20, 64)]),
}


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


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


class Parent:
    """cpk_encode_batch of another build of the library, through its own context."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(str(path))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        self.lib.cpk_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.cpk_ctx_destroy.argtypes = [vp]
        self.lib.cpk_ctx_destroy.restype = None
        self.lib.cpk_encode_batch.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp]
        self.h = vp()
        assert self.lib.cpk_ctx_create(0, ctypes.byref(self.h)) == 0

    def encode_batch(self, d_in, d_swo, maxw, d_out, d_off):
        rc = self.lib.cpk_encode_batch(self.h, d_in.data_ptr(), d_swo.data_ptr(), d_swo.numel() - 1, maxw,
                                       d_out.data_ptr(), d_off.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def close(self):
        self.lib.cpk_ctx_destroy(self.h)


def row(ctx, parent, name, reps):
    cfg, shape = ROWS[name]
    i64 = dict(dtype=torch.int64, device="cuda")
    sizes = torch.cat([torch.full((k,), w, **i64) for k, w in shape])
    n, maxw = sizes.numel(), max(w for _, w in shape)
    d_swo = torch.cat([torch.zeros(1, **i64), torch.cumsum(sizes, 0)])
    words = int(d_swo[-1].item())
    d_in = torch.empty(words, **i64)
    ctx.generate(cp.preset(cfg), d_swo, d_in)
    torch.cuda.synchronize()
    d_soff = torch.zeros(n + 1, **i64)
    t_size = timed(lambda: ctx.packed_size_batch(d_in, d_swo, maxw, d_soff), reps)
    ok = ctx.take_error() == cp.OK
    total = int(d_soff[-1].item())
    print(f"{name}: preset {cfg}, {n} pieces ({' + '.join(f'{k} x {w}' for k, w in shape)} words), "
          f"{8.0 * words / (1 << 30):.3f} GiB unpacked, {total / (1 << 30):.3f} GiB packed", flush=True)
    # the encode that places for itself
    d_ref = torch.empty(int(cp.batch_capacity(d_swo.cpu().numpy())), dtype=torch.uint8, device="cuda")
    d_eoff = torch.zeros(n + 1, **i64)
    enc = parent if parent else ctx
    t_enc = timed(lambda: enc.encode_batch(d_in, d_swo, maxw, d_ref, d_eoff), reps)
    ok &= bool((d_eoff == d_soff).all().item())
    # size -> placed encode into exactly `total` bytes
    d_poff, d_glen = torch.zeros(n, **i64), torch.zeros(n, **i64)
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_out = torch.empty(total + 16 * n + 16, dtype=torch.uint8, device="cuda")
    t_at = timed(lambda: ctx.encode_batch_at(d_in, d_swo, maxw, None, d_out, total, d_soff, None, d_poff, d_glen,
                                             d_st), reps)
    mism, step = 0, 1 << 28
    for a in range(0, total, step):
        mism += int((d_out[a:min(a + step, total)] != d_ref[a:min(a + step, total)]).sum().item())
    bad = int((d_st != 0).sum().item()) + int((d_poff != d_soff[:n]).sum().item())
    # ... and with 16 bytes of room in front of every piece
    d_goff = d_soff[:n] + 16 * torch.arange(1, n + 1, **i64)
    t_gap = timed(lambda: ctx.encode_batch_at(d_in, d_swo, maxw, None, d_out, total + 16 * n, d_goff, None, d_poff,
                                              d_glen, d_st), reps)
    gbad = (int((d_st != 0).sum().item()) + int((d_poff != d_goff).sum().item()) +
            int((d_glen != d_soff[1:] - d_soff[:n]).sum().item()))
    ok &= mism == 0 and bad == 0 and gbad == 0
    which = "parent library" if parent else "this library (no --parent-lib)"
    print(f"    encode   {fmt(t_enc)}  cpk_encode_batch, {which}", flush=True)
    print(f"    size     {fmt(t_size)}", flush=True)
    print(f"    at       {fmt(t_at)}  mismatch = {mism} bytes, {bad} statuses / offsets", flush=True)
    print(f"    size+at  {t_size[0] + t_at[0]:9.3f} ms  = {(t_size[0] + t_at[0]) / t_enc[0]:.3f} of the encode", flush=True)
    print(f"    at+16    {fmt(t_gap)}  size+at+16 {t_size[0] + t_gap[0]:9.3f} ms, mismatch = {gbad} statuses / "
          f"lengths / offsets", flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="p2,p3,p4,dominant,tiny")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="another build of the library for the encode column")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    ctx = cp.Context(0)
    parent = Parent(a.parent_lib) if a.parent_lib else None
    ok = True
    try:
        for name in a.rows.split(","):
            ok &= row(ctx, parent, name, a.reps)
            torch.cuda.empty_cache()
    finally:
        ctx.close()
        if parent:
            parent.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
