"""The size query against the encode it spares, device-resident:
python tools/bench_packed_size.py [--pieces 1048576] [--piece-words 8192]
                                  [--presets 2,3,4] [--reps 10] [--encode-ms a,b,c]

For each preset a batch of --pieces pieces of --piece-words words is generated
on the device (cpk_generate), then timed with HIP events on the current stream
over --reps repeats after one warm-up (the median is printed, with the spread):

  size     cpk_packed_size_batch: milliseconds, GiB/s of unpacked words, the
           fraction of the read ceiling (--ceiling-gibs, the stream-read figure
           of profiles/r5Z_stream_mix.txt), and its ratio to the encode
  encode   cpk_encode_batch on the same input into a worst-case buffer.
           --encode-ms gives the encode times of another build (one per
           preset, e.g. the parent commit's run of this tool with
           CPK_LIB=<its library>) for the ratio instead; --no-encode skips
           the encode and its buffer (then no mismatch check either)

and the size call's offsets are compared with the encoder's (mismatch = 0).
CPK_SIZE_FORM=chunk / wave forces the size query's form for an A/B of its
gate.  Not part of bench.py.
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402


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


def case(ctx, cfg, n, pw, reps, encode, encode_ms, ceiling):
    i64 = dict(dtype=torch.int64, device="cuda")
    d_swo = torch.arange(n + 1, **i64) * pw
    d_in = torch.empty(n * pw, **i64)
    ctx.generate(cp.preset(cfg), d_swo, d_in)
    torch.cuda.synchronize()
    d_soff = torch.zeros(n + 1, **i64)
    t_s = timed(lambda: ctx.packed_size_batch(d_in, d_swo, pw, d_soff), reps)
    ok = ctx.take_error() == cp.OK
    total = int(d_soff[-1].item())
    u_gib = 8.0 * n * pw / (1 << 30)
    gibs = u_gib / (t_s[0] * 1e-3)

    def fmt(t):
        return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    print(f"config {cfg}: {n} pieces of {pw} words, {u_gib:.2f} GiB unpacked, {total / (1 << 30):.2f} GiB packed",
          flush=True)
    mism = None
    t_e = None
    if encode:
        cap = n * cp.packed_bound(pw) + 16
        d_pk = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_eoff = torch.zeros(n + 1, **i64)
        t_e = timed(lambda: ctx.encode_batch(d_in, d_swo, pw, d_pk, d_eoff), reps)
        ok &= ctx.take_error() == cp.OK
        mism = int((d_eoff != d_soff).sum().item())
        ok &= mism == 0
        del d_pk
    ref = encode_ms if encode_ms is not None else (t_e[0] if t_e else None)
    ratio = f"{t_s[0] / ref:.3f} of the encode's {ref:.3f} ms" if ref else "no encode time"
    print(f"    size   {fmt(t_s)}  {gibs:8.1f} GiB/s of U  {gibs / ceiling:.2f} of the {ceiling:.0f} GiB/s read ceiling"
          f"  ratio {ratio}", flush=True)
    if t_e:
        print(f"    encode {fmt(t_e)}  offsets mismatch = {mism}", flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=1 << 20)
    ap.add_argument("--piece-words", type=int, default=8192)
    ap.add_argument("--presets", default="2,3,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--encode-ms", default=None, help="encode milliseconds of another build, one per preset")
    ap.add_argument("--no-encode", action="store_true")
    ap.add_argument("--ceiling-gibs", type=float, default=5389.5,
                    help="the measured stream-read ceiling, GiB/s (5786.9 GB/s, profiles/r5Z_stream_mix.txt)")
    a = ap.parse_args()
    presets = [int(x) for x in a.presets.split(",")]
    enc_ms = [float(x) for x in a.encode_ms.split(",")] if a.encode_ms else [None] * len(presets)
    print("device:", torch.cuda.get_device_name(0), flush=True)
    ctx = cp.Context(0)
    ok = True
    try:
        for cfg, e in zip(presets, enc_ms):
            ok &= case(ctx, cfg, a.pieces, a.piece_words, a.reps, not a.no_encode, e, a.ceiling_gibs)
            torch.cuda.empty_cache()
    finally:
        ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
