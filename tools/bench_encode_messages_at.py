"""One packed message per slot, three ways:
python tools/bench_encode_messages_at.py [--parent-lib PATH] [--reps 10] [--scale 1.0]

  a  tiled    cpk_encode_messages (the parent's library when given): the
              messages back to back, no slots -- the floor
  b  batch_at what a caller does without the new call: cpk_encode_batch_at
              (the parent's library when given) with the table words built on
              the host and put into d_in as each group's first piece; the host
              time to build them is reported apart and is not in the median
  c  msgs_at  cpk_encode_messages_at, the form unset, forced wave, forced place

over (1) 32,768 messages of 4 segments of 512..32,768 words, preset 3, each
slot behind a 4-byte gap; (2) 1 Mi messages of one 64-word segment, preset 2;
(3) 1,024 such small messages and one whose last segment is 8 Mi words.
--scale shrinks the message counts of (1) and (2).

Device resident, HIP events, the median of --reps after a warm-up, three runs
per arm interleaved in one process.  Every arm's bytes are checked: the slots
of b and c hold the same bytes buffer for buffer, every length equals a's, and
a sample of messages (the first, the last, the largest, 29 seeded) equals
oracle.write_message in a and in c; `mismatch` counts what differs.  Not part
of bench.py."""
import argparse
import ctypes
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "capnproto-java_amd"), str(REPO / "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import capnp_packed as cp  # noqa: E402
import oracle  # noqa: E402

I64 = dict(dtype=torch.int64, device="cuda")


def context(env=None, lib=None):
    """A context created under `env`; lib: another build of the library."""
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        if lib is None:
            return cp.Context(0)
        L = ctypes.CDLL(str(lib))
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        L.cpk_ctx_create.argtypes, L.cpk_ctx_destroy.argtypes = [i32, ctypes.POINTER(vp)], [vp]
        L.cpk_encode_messages.argtypes = [vp, vp, vp, u32, vp, u32, u64, vp, vp, vp]
        L.cpk_encode_batch_at.argtypes = [vp, vp, vp, u32, u64, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp]
        c = cp.Context.__new__(cp.Context)
        h = vp()
        assert L.cpk_ctx_create(0, ctypes.byref(h)) == 0
        c._lib, c.handle, c.device, c.decoder_forced = L, h, 0, False
        return c
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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
    return float(np.median(ts))


def host_tables(sizes, mseg):
    """The table words of every message and d_in's layout with them as the
    groups' first pieces -> (table words per message, flat table words)."""
    nm = len(mseg) - 1
    count = np.diff(mseg).astype(np.int64)
    tw = ((count + 2) & ~1) // 2
    toff = np.concatenate([[0], np.cumsum(tw)])
    ints = np.zeros(2 * int(toff[-1]), np.uint32)
    ints[2 * toff[:-1]] = (count - 1).astype(np.uint32)
    pos = np.repeat(2 * toff[:-1] + 1 - mseg[:-1].astype(np.int64), count) + np.arange(len(sizes))
    ints[pos] = sizes.astype(np.uint32)
    return tw, ints.view(np.uint64), nm


def shape(ctxs, label, sizes, mseg, cfg, gap, reps):
    nm, nseg = len(mseg) - 1, len(sizes)
    maxw = int(sizes.max())
    swo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_swo, d_mseg = torch.from_numpy(swo).cuda(), torch.from_numpy(mseg.astype(np.int64)).cuda()
    d_in = torch.empty(int(swo[-1]) + 8, **I64)
    ctxs["new"].generate(cp.preset(cfg), d_swo, d_in)
    # ---- a: tiled
    cap = cp.batch_capacity(swo.astype(np.uint64)) + 2100 * nm + 64
    d_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_aoff = torch.zeros(nm + nseg + 1, **I64)
    run_a = lambda: ctxs["parent"].encode_messages(d_in, d_swo, d_mseg, maxw, d_a, d_aoff)
    run_a()
    torch.cuda.synchronize()
    aoff = d_aoff.cpu().numpy()
    first = (mseg[:-1] + np.arange(nm)).astype(np.int64)
    mstart = np.concatenate([aoff[first], aoff[-1:]])
    mlen = np.diff(mstart)
    dst = mstart[:-1] + gap * (np.arange(nm) + 1)
    out_cap = int(dst[-1] + mlen[-1]) + 16
    d_dst, d_cap = torch.from_numpy(dst).cuda(), torch.from_numpy(mlen).cuda()
    # ---- b: the tables built on the host, as each group's first piece
    t0 = time.perf_counter()
    tw, twords, _ = host_tables(sizes, mseg)
    psizes = np.insert(sizes.astype(np.int64), mseg[:-1].astype(np.int64), tw)  # (table, then the segments)
    pswo = np.concatenate([[0], np.cumsum(psizes)])
    grp = (mseg + np.arange(nm + 1)).astype(np.int64)
    host_ms = 1e3 * (time.perf_counter() - t0)
    d_pswo, d_grp = torch.from_numpy(pswo).cuda(), torch.from_numpy(grp).cuda()
    d_in2 = torch.empty(int(pswo[-1]) + 8, **I64)
    is_t = np.zeros(nm + nseg, bool)
    is_t[grp[:-1]] = True
    tpos = np.repeat(pswo[:-1][is_t], tw) + (np.arange(int(tw.sum())) - np.repeat(np.cumsum(tw) - tw, tw))
    d_in2[torch.from_numpy(tpos).cuda()] = torch.from_numpy(twords.view(np.int64)).cuda()
    spos = torch.from_numpy(pswo[:-1][~is_t]).cuda()
    seg_of = torch.repeat_interleave(torch.arange(nseg, device="cuda"), torch.from_numpy(sizes.astype(np.int64)).cuda())
    idx = torch.arange(int(swo[-1]), device="cuda")
    d_in2[spos[seg_of] + idx - d_swo[:-1][seg_of]] = d_in[:int(swo[-1])]
    del seg_of, idx
    d_b = torch.zeros(out_cap, dtype=torch.uint8, device="cuda")
    b_poff, b_len = torch.zeros(nm + nseg, **I64), torch.zeros(nm, **I64)
    b_st = torch.zeros(nm, dtype=torch.int32, device="cuda")
    run_b = lambda: ctxs["parent"].encode_batch_at(d_in2, d_pswo, max(maxw, 257), d_grp, d_b, out_cap, d_dst, d_cap,
                                                   b_poff, b_len, b_st)
    # ---- c: the new call
    arms = {"a tiled": run_a, "b batch_at": run_b}
    bufs = {}
    for name in ("unset", "wave", "place"):
        d_c = torch.zeros(out_cap, dtype=torch.uint8, device="cuda")
        c_poff, c_len = torch.zeros(nm + nseg, **I64), torch.zeros(nm, **I64)
        c_st = torch.zeros(nm, dtype=torch.int32, device="cuda")
        bufs[name] = (d_c, c_len, c_st)
        arms[f"c msgs_at {name}"] = (lambda x=ctxs[name], o=d_c, p=c_poff, n=c_len, st=c_st:
                                     x.encode_messages_at(d_in, d_swo, d_mseg, maxw, o, out_cap, d_dst, d_cap, p, n, st))
    runs = {k: [] for k in arms}
    for _ in range(3):  # (interleaved)
        for k, f in arms.items():
            runs[k].append(timed(f, reps))
    torch.cuda.synchronize()
    # ---- the bytes
    d_len = torch.from_numpy(mlen).cuda()
    mism = {"b batch_at": int((b_len != d_len).sum()) + int((b_st != 0).sum())}
    for name, (d_c, c_len, c_st) in bufs.items():
        mism[f"c msgs_at {name}"] = int((c_len != d_len).sum()) + int((c_st != 0).sum()) + int(not torch.equal(d_c, d_b))
    rng = np.random.default_rng(3)
    sample = sorted({0, nm - 1, int(np.argmax(mlen))} | {int(i) for i in rng.integers(0, nm, size=29)})
    bad_a = 0
    for m in sample:
        s0, s1 = int(mseg[m]), int(mseg[m + 1])
        segs = [d_in[int(swo[s]):int(swo[s + 1])].cpu().numpy().tobytes() for s in range(s0, s1)]
        want = oracle.write_message(segs)
        bad_a += d_a[int(mstart[m]):int(mstart[m + 1])].cpu().numpy().tobytes() != want
        for name, (d_c, _, _) in bufs.items():
            mism[f"c msgs_at {name}"] += d_c[int(dst[m]):int(dst[m]) + len(want)].cpu().numpy().tobytes() != want
    mism["a tiled"] = int(bad_a)
    words = int(swo[-1])
    print(f"({label}) {nm} messages, {nseg} segments, {8 * words / (1 << 20):.1f} MiB of words, "
          f"{int(mstart[-1]) / (1 << 20):.1f} MiB packed; host table build for b: {host_ms:.2f} ms", flush=True)
    for k in arms:
        r = runs[k]
        print(f"    {k:22s} {np.median(r):9.3f} ms  (runs {r[0]:.3f} {r[1]:.3f} {r[2]:.3f})  mismatch {mism[k]}", flush=True)
    return sum(mism.values()) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library for arms a and b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="1,2,3")
    a = ap.parse_args()
    oracle.build()
    print("device:", torch.cuda.get_device_name(0), "parent library:", a.parent_lib or "(this build)", flush=True)
    ctxs = {"new": context(), "parent": context(lib=a.parent_lib), "unset": context(),
            "wave": context({"CPK_MSG_AT_FORM": "wave"}), "place": context({"CPK_MSG_AT_FORM": "place"})}
    rng = np.random.default_rng(1)
    ok = True
    if "1" in a.shapes:
        nm = max(int(32768 * a.scale), 8)
        ok &= shape(ctxs, "1: 4 segments of 512..32768 words, preset 3", rng.integers(512, 32769, size=4 * nm),
                    np.arange(nm + 1) * 4, 3, 4, a.reps)
    if "2" in a.shapes:
        nm = max(int((1 << 20) * a.scale), 8)
        ok &= shape(ctxs, "2: one 64-word segment, preset 2", np.full(nm, 64), np.arange(nm + 1), 2, 4, a.reps)
    if "3" in a.shapes:
        sizes = np.concatenate([np.full(1024, 64), [64, 300, 8 << 20]])
        ok &= shape(ctxs, "3: 1,024 small messages and one with an 8 Mi-word last segment", sizes,
                    np.concatenate([np.arange(1025), [1027]]), 2, 4, a.reps)
    for c in ctxs.values():
        c.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
