"""A stream of packed single-segment messages (config-2 words) read three
ways: python tools/bench_message_stream.py [--mib 64] [--reps 10]
(--mib sizes the words at a packed ratio of 0.375; config 2 packs to 0.474, so
the default stream is 81 MiB packed -- the size is printed)

  stream   cpk_decode_message_stream: the boundaries found on the device
  loop     the only way without it: a host loop of cpk_read_message, d_info[1]
           read back per message (a stream sync), the remainder copied to an
           aligned buffer when the next message does not start on 16 bytes
  floor    cpk_decode_messages given the true message offsets

for (a) messages of 64 KiB / 0.375 of words (79 KiB packed) and (b) 1 KiB / 0.375.  Timed with
HIP events on the current stream over --reps repeats after one warm-up; the
median is printed, with the spread.  Not part of bench.py.
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402

LIMIT = 1 << 31


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


def case(ctx, label, seg_words, nm, reps, loop_reps):
    i64 = dict(dtype=torch.int64, device="cuda")
    swo = np.arange(nm + 1, dtype=np.uint64) * seg_words
    d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
    d_mso = torch.arange(nm + 1, **i64)
    words = nm * seg_words
    d_in = torch.empty(words, **i64)
    ctx.generate(cp.preset(2), d_swo, d_in)
    cap = cp.batch_capacity(swo) + 20 * nm + 64
    d_pk = torch.zeros((cap + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(2 * nm + 1, **i64)
    ctx.encode_messages(d_in, d_swo, d_mso, seg_words, d_pk, d_off)
    torch.cuda.synchronize()
    P = int(d_off[-1].item())
    d_moff = d_off[0::2].contiguous()  # message m starts at piece 2 m (its table)

    # ---- the new call
    flat = words + nm
    d_out = torch.zeros(flat, **i64)
    d_mo, d_ms = torch.zeros(nm + 1, **i64), torch.zeros(nm + 1, **i64)
    d_sb, d_sw = torch.zeros(nm, **i64), torch.zeros(nm, **i64)
    res = {}

    def stream():
        res["s"] = ctx.decode_message_stream(d_pk, P, d_out, d_mo, d_ms, d_sb, d_sw, LIMIT)
    t_s = timed(stream, reps)
    rc, info = res["s"]
    cnt = torch.zeros(1, **i64)
    got = d_out.view(nm, seg_words + 1)[:, 1:].contiguous()
    ctx.count_mismatch(d_in, got, words, cnt)
    ok_s = (rc == 0 and info == [nm, nm, flat, P, 0] and int(cnt.item()) == 0
            and torch.equal(d_mo, d_moff) and bool((d_sw == seg_words).all()))

    # ---- the host loop of cpk_read_message
    reach = 10 * (seg_words + cp.MSG_HEAD_WORDS) + 16
    d_one = torch.zeros(seg_words + cp.MSG_HEAD_WORDS, **i64)
    d_info = torch.zeros(cp.MSG_INFO_WORDS, **i64)
    d_tmp = torch.zeros((reach + 255) // 256 * 256 + 64, dtype=torch.uint8, device="cuda")
    seen = {}

    def loop():
        pos = n = 0
        while pos < P:
            avail = min(P - pos, reach)
            src = d_pk[pos:]
            if pos % 16:
                d_tmp[:avail].copy_(d_pk[pos:pos + avail])
                src = d_tmp
            ctx.read_message(src, avail, d_one, d_info, traversal_limit_words=LIMIT)
            st, used = (int(v) for v in d_info[:2].cpu())
            assert st == 0 and used > 0, (st, used, pos)
            pos += used
            n += 1
        seen["n"], seen["pos"] = n, pos
    t_l = timed(loop, loop_reps)
    ok_l = seen == {"n": nm, "pos": P}

    # ---- the floor: the true offsets given
    d_fout = torch.zeros(words, **i64)
    d_fswo, d_fsin = torch.zeros(nm + 1, **i64), torch.zeros(nm + 1, **i64)
    d_fsst = torch.zeros(nm, dtype=torch.int32, device="cuda")
    d_fms, d_fmst = torch.zeros(nm + 1, **i64), torch.zeros(nm, dtype=torch.int32, device="cuda")

    def floor():
        res["f"] = ctx.decode_messages(d_pk, d_moff, d_fout, d_fswo, d_fsin, d_fsst, d_fms, d_fmst, LIMIT)
    t_f = timed(floor, reps)
    cnt.zero_()
    ctx.count_mismatch(d_in, d_fout, words, cnt)
    ok_f = res["f"] == (0, words, nm) and int(cnt.item()) == 0 and bool((d_fmst == 0).all())

    def fmt(t):
        return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    print(f"({label}) {nm} messages of {seg_words} words, {P / (1 << 20):.1f} MiB packed, "
          f"{8 * words / (1 << 20):.1f} MiB of words", flush=True)
    print(f"    stream {fmt(t_s)} ok={ok_s}  {1e3 * t_s[0] / nm:.3f} us per message", flush=True)
    print(f"    loop   {fmt(t_l)} ok={ok_l}  {1e3 * t_l[0] / nm:.3f} us per message", flush=True)
    print(f"    floor  {fmt(t_f)} ok={ok_f}", flush=True)
    return ok_s and ok_l and ok_f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=64.0, help="packed size of the stream at a ratio of 0.375")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-reps", type=int, default=None, help="repeats of the host loop (default: --reps)")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    ctx = cp.Context(0)
    ok = True
    try:
        # (sized as if config-2 words packed to 0.375 of their size)
        for label, kib in (("a", 64), ("b", 1)):
            seg_words = int(kib * 1024 / 8 / 0.375)
            nm = int(a.mib * 1024 / kib)
            ok &= case(ctx, label, seg_words, nm, a.reps, a.loop_reps or a.reps)
    finally:
        ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
