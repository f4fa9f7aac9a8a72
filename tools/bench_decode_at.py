"""Placed decode against the decode of tiled pieces, device-resident:
python tools/bench_decode_at.py [--rows p2,p3,p4,tiny] [--runs 3] [--reps 10] [--gap 4]

Rows (each generated on the device, cpk_generate, packed by cpk_encode_batch):
  p2 p3 p4   131,072 pieces of 8192 words (64 KiB) at presets 2, 3 and 4
  tiny       1 Mi pieces of 64 words (preset 2)
Arms, HIP events on the current stream, the median of --reps repeats after one
warm-up; --runs runs per arm, interleaved in this process (batch, at, size,
batch, at, size, ...), so that the run-to-run range of each arm is seen beside
the difference between them:
  batch      cpk_decode_batch on the pieces tiled, as cpk_encode_batch left
             them
  at         cpk_decode_batch_at on the same pieces in slots with a prefix gap
             of --gap bytes (4) in front of each: d_src_off[i] = offset[i] +
             gap (i + 1), laid out by cpk_encode_batch_at.  (--gap 16 keeps
             every piece at the 16-byte phase it has when tiled: an A/B of
             the line phase of the piece starts.)
  size+at    cpk_unpacked_size_batch_at over the same slots, then the decode
             with the offsets it wrote
Every decode is compared with the words that were packed (mismatch = differing
words, 0 expected) and every status must be CPK_OK.  CPK_DECODER=1|2 forces
the decoder of all arms.  Not part of bench.py.
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402

ROWS = {"p2": (2, 131072, 8192), "p3": (3, 131072, 8192), "p4": (4, 131072, 8192), "tiny": (2, 1 << 20, 64)}


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
    return float(np.median(np.array(ts)))


def row(ctx, name, runs, reps, GAP):
    cfg, n, w = ROWS[name]
    i64 = dict(dtype=torch.int64, device="cuda")
    d_swo = torch.arange(n + 1, **i64) * w
    words = n * w
    d_in = torch.empty(words, **i64)
    ctx.generate(cp.preset(cfg), d_swo, d_in)
    # tiled: cpk_encode_batch; placed: the same pieces behind a 4-byte gap each
    d_tiled = torch.empty(int(cp.batch_capacity(d_swo.cpu().numpy())), dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, **i64)
    ctx.encode_batch(d_in, d_swo, w, d_tiled, d_off)
    torch.cuda.synchronize()
    total = int(d_off[-1].item())
    in_cap = total + GAP * n
    d_src = d_off[:n] + GAP * torch.arange(1, n + 1, **i64)
    d_len = torch.zeros(n, **i64)
    d_poff = torch.zeros(n, **i64)
    d_est = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_placed = torch.zeros((in_cap + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    ctx.encode_batch_at(d_in, d_swo, w, None, d_placed, in_cap, d_src, None, d_poff, d_len, d_est)
    torch.cuda.synchronize()
    ok = bool((d_est == 0).all().item()) and bool((d_len == d_off[1:] - d_off[:n]).all().item())
    print(f"{name}: gap {GAP}, preset {cfg}, {n} pieces of {w} words, {8.0 * words / (1 << 30):.3f} GiB unpacked, "
          f"{total / (1 << 30):.3f} GiB packed", flush=True)
    d_out = torch.empty(words, **i64)
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_gst = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_used = torch.zeros(n, **i64)
    d_sz = torch.zeros(n + 1, **i64)
    cnt = torch.zeros(1, **i64)

    def check(what):
        cnt.zero_()
        ctx.count_mismatch(d_in, d_out, words, cnt)
        bad = int(cnt.item()) + int((d_st != 0).sum().item())
        if bad:
            print(f"    {what}: {bad} words / statuses off", flush=True)
        d_out.zero_()
        return bad == 0

    def size_then_at():
        ctx.unpacked_size_batch_at(d_placed, in_cap, d_src, d_len, d_sz, d_st)
        ctx.decode_batch_at(d_placed, in_cap, d_src, d_len, None, d_sz, d_out, d_st, d_gst, d_used)

    arms = {
        "batch": lambda: ctx.decode_batch(d_tiled, d_off, d_swo, d_out, d_st),
        "at": lambda: ctx.decode_batch_at(d_placed, in_cap, d_src, d_len, None, d_swo, d_out, d_st, d_gst, d_used),
        "size+at": size_then_at,
    }
    t = {k: [] for k in arms}
    for _ in range(runs):
        for k, f in arms.items():
            t[k].append(timed(f, reps))
            ok &= check(k)
    for k, v in t.items():
        print(f"    {k:8s} " + "  ".join(f"{x:8.3f}" for x in v) + f"  ms   range {min(v):.3f}-{max(v):.3f}", flush=True)
    lo, hi = min(t["batch"]), max(t["batch"])
    inside = all(lo <= x <= hi for x in t["at"])
    print(f"    at inside batch's run-to-run range [{lo:.3f}, {hi:.3f}]: {inside}; "
          f"medians at / batch = {np.median(t['at']) / np.median(t['batch']):.4f}", flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="p2,p3,p4,tiny")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gap", type=int, default=4, help="bytes in front of every placed piece")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    ctx = cp.Context(0)
    ok = True
    try:
        for name in a.rows.split(","):
            ok &= row(ctx, name, a.runs, a.reps, a.gap)
            torch.cuda.empty_cache()
    finally:
        ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
