"""Messages decoded from placed slots against the same messages tiled,
device-resident:
python tools/bench_decode_messages_at.py [--messages 32768] [--runs 3] [--reps 10] [--gap 4]

The messages have bench.py's config-3 shape: 4 segments each, segment sizes
drawn from {512 .. 32768} words with bench.py's seed, words from the
generator's preset 3, packed by cpk_encode_messages (tables included).
Arms, HIP events on the current stream, the median of --reps repeats after one
warm-up; --runs runs per arm, interleaved in this process (tiled, placed,
tiled, placed, ...), so that the run-to-run range of each arm is seen beside
the difference between them:
  tiled    cpk_decode_messages on the messages as cpk_encode_messages left
           them (it synchronises the stream once, to read the totals)
  placed   cpk_decode_messages_at on the same messages in slots with a gap of
           --gap bytes (4) of 0xFF in front of each (no synchronisation)
Every decode is compared with the words that were packed (mismatch = differing
words, 0 expected), every message must be CPK_OK and the placed call's totals
those of the batch.  CPK_DECODER=1|2 forces the decoder of both arms.  Not
part of bench.py.
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402

SEED = 0x1D2ACD47  # bench.py's
SEG_WORDS = np.array([512, 1024, 2048, 4096, 8192, 16384, 32768], dtype=np.uint64)


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


def place(d_tiled, d_moff, nm, gap):
    """The tiled messages copied into slots, `gap` bytes of 0xFF in front of
    each: -> (buffer, d_src_off, d_src_len, in_cap).  A chunk of the buffer at
    a time: each byte looks its message up."""
    i64 = dict(dtype=torch.int64, device="cuda")
    total = int(d_moff[nm].item())
    d_src = d_moff[:nm] + gap * torch.arange(1, nm + 1, **i64)
    d_len = d_moff[1:] - d_moff[:nm]
    in_cap = total + gap * nm
    d_placed = torch.full(((in_cap + 15) // 16 * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    chunk = 1 << 27
    for p0 in range(0, in_cap, chunk):
        p = torch.arange(p0, min(p0 + chunk, in_cap), **i64)
        m = (torch.searchsorted(d_src, p, right=True) - 1).clamp_(min=0)
        src = p - gap * (m + 1)
        inside = (src >= d_moff[m]) & (src < d_moff[m + 1])
        d_placed[p0:p0 + p.numel()] = torch.where(inside, d_tiled[src.clamp_(0, total - 1)], 0xFF)
    return d_placed, d_src, d_len, in_cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=32768)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gap", type=int, default=4, help="bytes in front of every placed message")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    nm, n = a.messages, 4 * a.messages
    rng = np.random.default_rng(SEED)
    seg_words = SEG_WORDS[rng.integers(0, len(SEG_WORDS), size=n)]
    swo = np.concatenate([[0], np.cumsum(seg_words)]).astype(np.uint64)
    words = int(swo[-1])
    i64 = dict(dtype=torch.int64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    ctx = cp.Context(0)
    ok = True
    try:
        d_swo = torch.from_numpy(swo.astype(np.int64)).cuda()
        d_mso = torch.arange(0, n + 1, 4, **i64)
        d_in = torch.empty(words, **i64)
        ctx.generate(cp.preset(3), d_swo, d_in)
        cap = cp.batch_capacity(swo) + 40 * nm
        d_tiled = torch.empty((cap + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
        d_off = torch.empty(nm + n + 1, **i64)
        ctx.encode_messages(d_in, d_swo, d_mso, int(seg_words.max()), d_tiled, d_off)
        # message m starts at piece 5 m (its table), the last entry is the total
        d_moff = d_off[torch.arange(0, 5 * nm + 1, 5, **i64)].contiguous()
        torch.cuda.synchronize()
        d_placed, d_src, d_len, in_cap = place(d_tiled, d_moff, nm, a.gap)
        print(f"config-3 shape: gap {a.gap}, preset 3, {nm} messages x 4 segments, "
              f"{8.0 * words / (1 << 30):.3f} GiB unpacked, {int(d_moff[nm].item()) / (1 << 30):.3f} GiB packed",
              flush=True)
        d_out = torch.empty(words, **i64)
        d_sw, d_sin, d_sst = torch.zeros(n + 1, **i64), torch.zeros(n, **i64), torch.zeros(n, **i32)
        d_mseg, d_mst = torch.zeros(nm + 1, **i64), torch.zeros(nm, **i32)
        d_used, d_tot = torch.zeros(nm, **i64), torch.zeros(cp.MAT_TOTALS, **i64)
        cnt = torch.zeros(1, **i64)
        rcs = []

        def tiled():
            rcs.append(ctx.decode_messages(d_tiled, d_moff, d_out, d_sw, d_sin, d_sst, d_mseg, d_mst))

        def placed():
            ctx.decode_messages_at(d_placed, in_cap, d_src, d_len, d_out, d_sw, d_sin, d_sst, d_mseg, d_mst, d_used,
                                   d_tot)

        def check(what):
            cnt.zero_()
            ctx.count_mismatch(d_in, d_out, words, cnt)
            bad = int(cnt.item()) + int((d_mst != 0).sum().item()) + int((d_sst != 0).sum().item())
            if what == "tiled":
                bad += sum(1 for rc in rcs if rc != (cp.OK, words, n))
                rcs.clear()
            else:
                bad += [int(v) for v in d_tot.cpu()] != [words, n, nm]
                bad += int((d_used != d_len).sum().item())
            if bad:
                print(f"    {what}: {bad} words / statuses / totals off", flush=True)
            d_out.zero_()
            d_mst.fill_(1)
            d_sst.fill_(1)
            return bad == 0

        arms = {"tiled": tiled, "placed": placed}
        t = {k: [] for k in arms}
        for _ in range(a.runs):
            for k, f in arms.items():
                t[k].append(timed(f, a.reps))
                ok &= check(k)
        for k, v in t.items():
            print(f"    {k:8s} " + "  ".join(f"{x:8.3f}" for x in v) + f"  ms   range {min(v):.3f}-{max(v):.3f}",
                  flush=True)
        lo, hi = min(t["tiled"]), max(t["tiled"])
        inside = all(lo <= x <= hi for x in t["placed"])
        print(f"    placed inside tiled's run-to-run range [{lo:.3f}, {hi:.3f}]: {inside}; "
              f"medians placed / tiled = {np.median(t['placed']) / np.median(t['tiled']):.4f}", flush=True)
    finally:
        ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
