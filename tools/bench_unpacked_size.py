"""The unpacked-size query against the decode it precedes, device-resident:
python tools/bench_unpacked_size.py [--pieces 131072] [--piece-words 8192]
                                    [--presets 2,4,3] [--reps 10] [--sweep-mib 0.125,...,256]

Batches.  For presets 2 and 4 a batch of --pieces pieces of --piece-words
words, for preset 3 ragged message pieces (16 KiB pieces, every 64th of 1 MiB),
is generated on the device (cpk_generate) and packed (cpk_encode_batch); then
timed with HIP events on the current stream over --reps repeats after one
warm-up (the median is printed, with the spread):

  size     cpk_unpacked_size_batch on the packed ranges: milliseconds, GiB/s
           of packed bytes, the fraction of the read ceiling (--ceiling-gibs,
           the stream-read figure of profiles/r5Z_stream_mix.txt), and its
           ratio to the decode
  decode   cpk_decode_batch of the same batch with the offsets the size call
           wrote, in the same run

and the size call's offsets are compared with the words that were packed
(mismatch = 0).  The size query must be the faster of the two at every shape.

The one-piece sweep.  One piece of preset-2 data of about each --sweep-mib
packed MiB, through the block-map form (a context under CPK_USIZE_FORM=1), the
wave-per-piece form (CPK_USIZE_FORM=2), the default choice and cpk_decode_batch:
the crossover of the first two is the threshold in host_api.hip (kUsBlockMin).
Not part of bench.py.
"""
import argparse
import os
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


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


I64 = dict(dtype=torch.int64, device="cuda")


def packed_batch(ctx, cfg, sizes):
    """-> (d_packed, d_in_off, d_swo, packed bytes) of the pieces, generated and packed on the device."""
    n = len(sizes)
    d_swo = torch.cat([torch.zeros(1, **I64), torch.cumsum(torch.as_tensor(sizes, **I64), 0)])
    words = int(d_swo[-1].item())
    d_in = torch.empty(words, **I64)
    ctx.generate(cp.preset(cfg), d_swo, d_in)
    cap = int(sum(cp.packed_bound(int(s)) * int(c) for s, c in zip(*np.unique(sizes, return_counts=True))))
    d_pk = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, **I64)
    ctx.encode_batch(d_in, d_swo, int(max(sizes)), d_pk, d_off)
    assert ctx.take_error() == cp.OK
    return d_pk, d_off, d_swo, int(d_off[-1].item())


def batch_case(ctx, cfg, sizes, reps, ceiling, what):
    n = len(sizes)
    d_pk, d_off, d_swo, P = packed_batch(ctx, cfg, sizes)
    words = int(d_swo[-1].item())
    d_got = torch.zeros(n + 1, **I64)
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_out = torch.empty(words + 8, **I64)
    d_st2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_s = timed(lambda: ctx.unpacked_size_batch(d_pk, d_off, d_got, d_st), reps)
    t_d = timed(lambda: ctx.decode_batch(d_pk, d_off, d_got, d_out, d_st2), reps)
    mism = int((d_got != d_swo).sum().item()) + int((d_st != 0).sum().item()) + int((d_st2 != 0).sum().item())
    p_gib = P / (1 << 30)
    gibs = p_gib / (t_s[0] * 1e-3)
    print(f"config {cfg}: {n} pieces, {what}, {8.0 * words / (1 << 30):.2f} GiB unpacked, {p_gib:.2f} GiB packed",
          flush=True)
    print(f"    size   {fmt(t_s)}  {gibs:8.1f} GiB/s of P  {gibs / ceiling:.3f} of the {ceiling:.0f} GiB/s read ceiling"
          f"  ratio {t_s[0] / t_d[0]:.3f} of the decode", flush=True)
    print(f"    decode {fmt(t_d)}  mismatch = {mism}", flush=True)
    return mism == 0 and t_s[0] < t_d[0]


def forced(form):
    saved = os.environ.get("CPK_USIZE_FORM")
    os.environ["CPK_USIZE_FORM"] = form
    try:
        return cp.Context(0)
    finally:
        if saved is None:
            os.environ.pop("CPK_USIZE_FORM")
        else:
            os.environ["CPK_USIZE_FORM"] = saved


def sweep(ctx, mibs, reps, ceiling):
    cb, cw = forced("1"), forced("2")
    ok = True
    print("one piece of config-2 data: block map / wave per piece / default / decode, ms (median of the repeats)",
          flush=True)
    try:
        # (config 2 packs to about 0.6 of its words' bytes: the words for the wanted packed size)
        probe = packed_batch(ctx, 2, [1 << 17])
        per_word = probe[3] / float(1 << 17)
        del probe
        for mib in mibs:
            w = max(64, int(mib * (1 << 20) / per_word))
            d_pk, d_off, d_swo, P = packed_batch(ctx, 2, [w])
            d_got = torch.zeros(2, **I64)
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_out = torch.empty(w + 8, **I64)
            r = max(3, reps if P < (32 << 20) else 3)
            res = {}
            for name, c in (("block", cb), ("wave", cw), ("auto", ctx)):
                d_got.zero_()
                res[name] = timed(lambda: c.unpacked_size_batch(d_pk, d_off, d_got, d_st), r)
                ok &= bool((d_got == d_swo).all().item()) and int(d_st.item()) == 0
            t_d = timed(lambda: ctx.decode_batch(d_pk, d_off, d_swo, d_out, d_st), r)
            ok &= int(d_st.item()) == 0 and res["auto"][0] < t_d[0]
            gibs = P / (1 << 30) / (res["auto"][0] * 1e-3)
            print(f"    {P / (1 << 20):9.3f} MiB packed  block {res['block'][0]:9.3f} ({res['block'][1]:.3f}-"
                  f"{res['block'][2]:.3f})  wave {res['wave'][0]:9.3f} ({res['wave'][1]:.3f}-{res['wave'][2]:.3f})  "
                  f"auto {res['auto'][0]:9.3f}  decode {t_d[0]:9.3f} ({t_d[1]:.3f}-{t_d[2]:.3f})  "
                  f"auto {gibs:7.1f} GiB/s of P, {gibs / ceiling:.3f} of the ceiling", flush=True)
            del d_pk, d_out
            torch.cuda.empty_cache()
    finally:
        cb.close()
        cw.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=131072)
    ap.add_argument("--piece-words", type=int, default=8192)
    ap.add_argument("--presets", default="2,4,3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweep-mib", default="0.125,0.25,0.5,1,2,4,16,64,256")
    ap.add_argument("--ceiling-gibs", type=float, default=5389.5,
                    help="the measured stream-read ceiling, GiB/s (5786.9 GB/s, profiles/r5Z_stream_mix.txt)")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    ctx = cp.Context(0)
    ok = True
    try:
        for cfg in [int(x) for x in a.presets.split(",") if x]:
            if cfg == 3:
                # ragged message pieces: 16 KiB of words, every 64th piece 1 MiB, as many words as the other batches
                n = max(64, a.pieces * a.piece_words // (63 * 2048 + 131072) * 64)
                sizes = [131072 if i % 64 == 63 else 2048 for i in range(n)]
                ok &= batch_case(ctx, 3, sizes, a.reps, a.ceiling_gibs, "2048 words, every 64th 131072")
            else:
                ok &= batch_case(ctx, cfg, [a.piece_words] * a.pieces, a.reps, a.ceiling_gibs,
                                 f"{a.piece_words} words each")
            torch.cuda.empty_cache()
        mibs = [float(x) for x in a.sweep_mib.split(",") if x]
        if mibs:
            ok &= sweep(ctx, mibs, a.reps, a.ceiling_gibs)
    finally:
        ctx.close()
    print("size faster than decode at every shape, offsets equal:", ok, flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
