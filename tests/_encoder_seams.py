"""Unpacked pieces with one planted run, for the encoder seam tests (no GPU,
no pytest; tests/test_encoder_seams_corpus.py pins this file against the
oracle and the mask-algebra model, tests/test_gpu_encoder_seams.py feeds the
corpora to every encoder form).

The two-pass encoder (csrc/encode_v4.hip) walks a piece with one wave in
steps of 64 words (lane = word), takes the roles of a group of 64 steps
lane-parallel (lane = step), and lays the strings into a ring of kE4RingBytes
bytes.  Every edge of that geometry gets named cases here:

  step    a run's start / end on either side of a step edge (and of the
          single pass's 2048-word wave edge), the loads' PF / EPF batch edges
  group   the same at word 4096, runs over a whole group, the last 0xFF
          head 255 / 256 / 257 words before the group's end
  zcap    the 256-word cap head of a zero run at lane 0 / 31 / 32 / 63 and at
          a group's first and last word
  long    D/L stretches that enter a step at 191 / 192 / 193 words (the
          lane-parallel form's limit) and further on
  count   a head's count from this step's row and the four rows ahead
  ring    strings at the ring's last bytes, dense stretches at every
          obase % 16
  lines   pieces of 1..3 words that share 16-byte output lines
  sizes   rand_piece pieces at the step / group / prefetch sizes
  many    batches of 4095 .. 8193 tiny pieces (the scan's block edges)

Words, as in tests/_packed_size_cases.py: M, the background, is nonzero
with six zero bytes and resets every run state; Z is a zero word; D has all 8
bytes nonzero; L has exactly one zero byte.  D and L members carry random
nonzero bytes, so a lost or OR-ed byte shows.  A case is a piece of M with
one planted run, named seam/kind/position/length, e.g.
grp4096/dense+L/enter193@+0/len600.  What an encoder must produce is always
the oracle's answer; nothing here computes packed bytes by hand.
"""
from __future__ import annotations

import zlib
from functools import lru_cache
from pathlib import Path

import numpy as np

from _packed_records import parse_constant
from _packed_size_cases import BG

CSRC = Path(__file__).resolve().parents[1] / "capnproto-java_amd" / "csrc"

# ---- geometry ----------------------------------------------------------------
# Named constants, read from their declarations (an unparsable one raises).
_CONSTANTS = {
    "kE4RingBytes": "encode_v4.hip",
    "kE4Ov": "encode_v4.hip",
    "PF": "encode_v4.hip",
    "EPF": "encode_v4.hip",
    "kE4ScanThreads": "encode_v4.hip",
    "kE4ScanPer": "encode_v4.hip",
    "kE4ScanBlock": "encode_v4.hip",
    "kSpSmallWords": "encode_sp3.hip",
    "kSpSmallPieces": "encode_sp3.hip",
}


def parse_constants() -> dict:
    out = {}
    for name, src in _CONSTANTS.items():
        out[name] = parse_constant((CSRC / src).read_text(), name, out)
    return out


CONST = parse_constants()
kE4RingBytes, kE4Ov, PF, EPF = CONST["kE4RingBytes"], CONST["kE4Ov"], CONST["PF"], CONST["EPF"]
kE4ScanBlock = CONST["kE4ScanBlock"]
kSpSmallWords, kSpSmallPieces = CONST["kSpSmallWords"], CONST["kSpSmallPieces"]

# The kernel's unnamed constants, each with the line it was read from and the
# text that line must still hold (check_pins): a change to the kernel fails
# the CPU test instead of silently moving the seam.
STEP = 64            # words per step: lane = word
GROUP_STEPS = 64     # encode_v4.hip:333  a group's roles are taken every 64 steps
GROUP = STEP * GROUP_STEPS
LONG = 192           # encode_v4.hip:210  a D/L stretch entering a step longer than this is taken by sp_roles
ZCAP = 256           # encode_v4.hip:229  a zero run's cap head every 256 words, by phase
HD_CAP = 256         # encode_v4.hip:184  the distance back to the last 0xFF head, capped
LOOK_ROWS = 4        # encode_v4.hip:504  rows of look-ahead for a head's count
COUNT_CAP = 255      # encode_v4.hip:508  a head's count
FLUSH_LINES = 64     # encode_v4.hip:547  complete lines per flush
WAVE = 2048          # encode_sp.hip: the single pass's wave of 32 steps
PINS = (
    ("encode_v4.hip", 333, "if (((s0 + PF) & 63) == 0 || s0 + PF >= nsteps) {"),
    ("encode_v4.hip", 337, "const int cnt = (int)min(64u, nsteps - g0);"),
    ("encode_v4.hip", 210, "const bool longc = cont && len > 192;"),
    ("encode_v4.hip", 229, "const uint32_t j0 = (256u - (zl & 255u)) & 255u;"),
    ("encode_v4.hip", 184, "st.hd = (uint32_t)min(P - h, 256);"),
    ("encode_v4.hip", 285, "(w0 - swo[0]) / 64 + seg"),
    ("encode_v4.hip", 504, ": bv4 ? 192u + (uint32_t)__builtin_ctzll(bv4) : 256u;"),
    ("encode_v4.hip", 507, "const uint32_t z_hi = sp_ffbl((uint32_t)(e >> 32)) | 32u;"),
    ("encode_v4.hip", 508, "min((uint32_t)(63 - lane) + X, 255u)"),
    ("encode_v4.hip", 547, "if ((uint32_t)(rpos >> 4) - (uint32_t)fl >= 64u) {"),
    ("encode_v4.hip", 607, "(f == 0 ? ~0ull : 0ull)"),
    ("host_pipe.hip", 233, "words <= cpk::kSpSmallWords && np <= cpk::kSpSmallPieces && !getenv(\"CPK_NO_SMALL\")"),
)


def check_pins():
    """Every pinned line still holds its text."""
    for src, line, text in PINS:
        lines = (CSRC / src).read_text().splitlines()
        assert line <= len(lines) and text in lines[line - 1], f"{src}:{line} no longer reads {text!r}"


# Bytes one GPU call may move (the limit tests/test_packed_records.py holds
# the decoder corpora to): asserted for every corpus when it is built.
LIMIT_PACKED, LIMIT_WORDS = 64 << 20, 256 << 20


# ---- words ---------------------------------------------------------------------
def _rng(*key) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bg(n: int) -> np.ndarray:
    """n background words, as an (n, 8) byte array."""
    return np.tile(BG, (n, 1))


def dense(rng, n: int) -> np.ndarray:
    return rng.integers(1, 256, size=(n, 8), dtype=np.uint8)


def lonely(rng, n: int) -> np.ndarray:
    w = dense(rng, n)
    w[np.arange(n), rng.integers(0, 8, size=n)] = 0
    return w


KINDS = ("zero", "dense", "dense+L", "L")


def run_words(kind: str, n: int, rng, dpos: int = 0) -> np.ndarray:
    """n words of one planted run.
    zero     Z words
    dense    D words: a head every 256
    dense+L  D words, every third an L (a literal-run member that is no head)
    L        L words only: a D/L stretch with no head
    D+L      one D, then L members
    L+D      L words with one D at dpos: no head before it"""
    if kind == "zero":
        return np.zeros((n, 8), np.uint8)
    if kind == "dense":
        return dense(rng, n)
    if kind == "dense+L":
        w = dense(rng, n)
        w[2::3] = lonely(rng, len(w[2::3]))
        return w
    w = lonely(rng, n)
    if kind == "D+L":
        w[0] = dense(rng, 1)
    elif kind == "L+D":
        w[dpos] = dense(rng, 1)
    else:
        assert kind == "L", kind
    return w


def word_classes(words: np.ndarray) -> str:
    """One letter per word: Z, D, L, or M for anything else."""
    nz = (np.asarray(words, np.uint8).reshape(-1, 8) != 0).sum(axis=1)
    code = np.full(nz.size, ord("M"), np.uint8)
    code[nz == 0] = ord("Z")
    code[nz == 8] = ord("D")
    code[nz == 7] = ord("L")
    return code.tobytes().decode()


class Case:
    """A piece: name, its bytes (uint8, a whole number of words), the corpus
    family, and what the builder planted: kind, start, length (words), and
    per family at (the named edge), enter, cap (the cap head's word), head,
    count, prefix (words before a ring probe), k."""
    __slots__ = ("name", "words", "family", "meta")

    def __init__(self, name, family, words, **meta):
        self.name, self.family, self.meta = name, family, meta
        self.words = np.ascontiguousarray(words, np.uint8).reshape(-1)
        assert self.words.size % 8 == 0

    @property
    def nwords(self):
        return self.words.size // 8


def _planted(name, family, W, start, kind, length, dpos=0, **meta) -> Case:
    assert 0 <= start and start + length <= W, (name, W, start, length)
    w = bg(W)
    w[start:start + length] = run_words(kind, length, _rng(name), dpos)
    return Case(name, family, w, kind=kind, start=start, length=length, **meta)


def _fit(least: int, residue: int) -> int:
    """The smallest W >= least with W % 64 == residue."""
    return least + (residue - least) % STEP


# ---- families --------------------------------------------------------------------
STEP_K = (1, 3, 4, 5, 8, 9)   # 64 k: either side of the EPF (4) and PF (8) load batches
WAVE_K = (1, 3)               # 2048 k: the single pass's wave edges inside one unit
EDGE_D = (-2, -1, 0, 1)
EDGE_LEN = (1, 2, 63, 64, 65)
TAILS = (7, 64, 70)           # background words after the run, cycling


def _edge_cases(seam: str, family: str, edges):
    """A run's start and its end (the first word after it) at edge + d."""
    out, i = [], 0
    for at in edges:
        for kind in KINDS:
            for d in EDGE_D:
                for side in ("start", "end"):
                    for ln in EDGE_LEN:
                        s = at + d if side == "start" else at + d - ln
                        if s < 0:
                            continue
                        W = s + ln + TAILS[i % 3]
                        i += 1
                        out.append(_planted(f"{seam}/{kind}/{side}@{at}{d:+d}/len{ln}", family, W, s, kind, ln,
                                            at=at, d=d, side=side))
    return out


def step_cases():
    return _edge_cases("step64", "step", [STEP * k for k in STEP_K]) + \
        _edge_cases("step2048", "step", [WAVE * k for k in WAVE_K])


COVER_A, COVER_B = (1, 64, 300), (1, 65, 300)
HEAD_BACK = (255, 256, 257)


def group_cases():
    out = _edge_cases("grp4096", "group", [GROUP])
    W = 3 * GROUP + 1
    # a run over the whole second group and more: every lane of that group
    # takes the kz < 0 / kd < 0 arm (the state entering the group)
    for kind in KINDS:
        for a in COVER_A:
            for b in COVER_B:
                ln = a + GROUP + b
                out.append(_planted(f"grp4096/{kind}/cover-{a}+{b}/len{ln}", "group", W, GROUP - a, kind, ln,
                                    at=GROUP, cover=(a, b)))
    # the last 0xFF head of the first group x words before its end (D+L: it
    # stays the last one; dense: the next head follows 256 words on)
    for kind in ("dense", "dense+L", "D+L"):
        for x in HEAD_BACK:
            for ln in (x + 100, x + 600):
                out.append(_planted(f"grp4096/{kind}/head@-{x}/len{ln}", "group", GROUP + 700, GROUP - x, kind, ln,
                                    at=GROUP, back=x))
    return out


ZCAP_LEN = (255, 256, 257, 511, 512, 513, 769)
ZCAP_LANES = (0, 63, 31, 32)


def zcap_cases():
    out, i = [], 0
    for lane in ZCAP_LANES:
        cap = STEP * 6 + lane
        for ln in ZCAP_LEN:
            s = cap - ZCAP
            out.append(_planted(f"zcap/zero/cap@step6.lane{lane}/len{ln}", "zcap", s + ln + TAILS[i % 3], s, "zero",
                                ln, cap=cap if ln > ZCAP else None))
            i += 1
    # the first and the second cap head on a group's last and first word
    for nth in (1, 2):
        for d in (-1, 0):
            for ln in (257, 513, 769):
                if ln <= nth * ZCAP:
                    continue
                cap = GROUP + d
                s = cap - nth * ZCAP
                out.append(_planted(f"zcap/zero/cap{nth}@4096{d:+d}/len{ln}", "zcap", s + ln + TAILS[i % 3], s,
                                    "zero", ln, cap=cap))
                i += 1
    # the run covers the whole second group: the phase reaches every lane of
    # it through st.zl, the cap head on that group's last word / the next
    # one's first (the run starts 16 or 17 caps before it: on the first
    # group's last words, or 256 words earlier)
    for d in (-1, 0):
        for back in (16, 17):
            cap = 2 * GROUP + d
            s = cap - ZCAP * back
            ln = 2 * GROUP + 300 - s
            out.append(_planted(f"zcap/zero/carried-from{s}/cap@8192{d:+d}/len{ln}", "zcap", 3 * GROUP + 1, s,
                                "zero", ln, cap=cap))
    return out


LONG_ENTER = (191, 192, 193, 224, 255, 256, 257)
LONG_KINDS = ("dense", "D+L", "L+D")


def long_cases():
    """D/L stretches that are `enter` words long where they enter the step at
    word 320 / the group at word 4096.  dense: the next head, 256 words after
    the first, lands at lane 65 / 64 / 63 / 32 / 1 / 0 of the entered step
    (65, 64: the step after) or, enter257, was its predecessor's last word.
    L+D: no head when the step is entered; the D comes ten words in."""
    out = []
    for seam, at in (("step320", 5 * STEP), ("grp4096", GROUP)):
        for kind in LONG_KINDS:
            for e in LONG_ENTER:
                for ln in (e + 70, 600):
                    s = at - e
                    out.append(_planted(f"{seam}/{kind}/enter{e}@+0/len{ln}", "long", s + ln + 70, s, kind, ln,
                                        dpos=e + 10, at=at, enter=e))
    return out


COUNT_LANES = (0, 31, 32, 63)
COUNT_STEP = 2
COUNT_W = (512, 513, 575)   # W % 64 in {0, 1, 63}


def count_cases():
    """A head (zero / 0xFF) at lane h of step 2 whose run is n words: the
    count is min(n - 1, 255).  n puts the run's end (the first word after
    it) in the same step on either side of bit 31 / 32 of the emit pass's
    `e`, on the first and last word of steps +1 .. +5, and 255 / 256 / 257
    words after the head.  Then the head in each of the piece's last five
    steps with the run reaching the piece's end (the emit pass reads rows
    past the piece's end as all boundaries)."""
    out, i = [], 0
    for kind, tag in (("zero", "zero"), ("dense", "ff")):
        for h in COUNT_LANES:
            head = STEP * COUNT_STEP + h
            ns = {1, 2, 255, 256, 257}
            ns |= {n for n in (31, 32, 33, 34, 63 - h) if 0 < n and h + n <= 63}
            for j in range(1, 6):
                ns |= {STEP * (COUNT_STEP + j) - head, STEP * (COUNT_STEP + j) + 63 - head}
            for n in sorted(ns):
                W = _fit(head + n + 2, (0, 1, 63)[i % 3])
                i += 1
                out.append(_planted(f"count/{tag}/head@step2.lane{h}/run{n}", "count", W, head, kind, n,
                                    head=head, count=min(n - 1, COUNT_CAP)))
        for W in COUNT_W:
            last = (W + 63) // 64 - 1
            for j in range(5):
                for h in COUNT_LANES:
                    head = STEP * (last - j) + h
                    if head >= W:
                        continue
                    n = W - head
                    out.append(_planted(f"count/{tag}/head@last-{j}.lane{h}/toend/W{W}", "count", W, head, kind, n,
                                        head=head, count=min(n - 1, COUNT_CAP)))
    return out


def _pad_words(nbytes: int, rng) -> np.ndarray:
    """Background and L words that pack to exactly nbytes (>= 14): an M word
    packs to 3 bytes, an L word outside a literal run to 8.  The M words come
    first, so whatever precedes them ends its run there."""
    assert nbytes >= 14, nbytes
    b = (3 * nbytes) % 8
    a = (nbytes - 3 * b) // 8
    assert a >= 0 and 8 * a + 3 * b == nbytes
    return np.concatenate([bg(b), lonely(rng, a)])


RING_K = tuple(range(1, 12))
RING_PROBES = ("ff10", "z2", "mem8")
RING_ROUNDS = (1, 3)
RING_DENSE = 800   # words: over three ring lengths at 8 bytes per word


def ring_cases():
    """One batch, in order.  Position cases: a prefix of M and L words whose
    packed length (the oracle's) is 2048 r - k, then the probe string -- a
    10-byte 0xFF head (D, then M), a 2-byte zero head (Z, then M) or an
    8-byte run member (D L, the prefix ending with the D) -- and a suffix that
    brings the piece to a multiple of 2048 packed bytes, so that in this
    batch every position case starts at obase % 2048 == 0 and the string
    lies at ring offset 2048 - k.  Then dense stretches of 800 words, each
    after a filler piece that sets its obase % 16."""
    import oracle
    out = []
    for r in RING_ROUNDS:
        for probe in RING_PROBES:
            for k in RING_K:
                name = f"ring/{probe}/ring@{kE4RingBytes}-{k}/round{r}"
                rng = _rng(name)
                target = kE4RingBytes * r - k
                head = dense(rng, 1) if probe == "mem8" else np.zeros((0, 8), np.uint8)
                prefix = np.concatenate([_pad_words(target - 10 * len(head), rng), head])
                P = len(oracle.pack(prefix.reshape(-1)))
                assert P % kE4RingBytes == kE4RingBytes - k, (name, P)
                body = {"ff10": dense(rng, 1), "z2": np.zeros((1, 8), np.uint8), "mem8": lonely(rng, 1)}[probe]
                sofar = np.concatenate([prefix, body, bg(1)])
                Q = len(oracle.pack(sofar.reshape(-1)))
                pad = (-Q) % kE4RingBytes
                pad += kE4RingBytes if pad < 14 else 0
                words = np.concatenate([sofar, _pad_words(pad, rng)])
                total = len(oracle.pack(words.reshape(-1)))
                assert total % kE4RingBytes == 0, (name, total)
                out.append(Case(name, "ring", words, kind=probe, prefix=len(prefix), k=k, packed=total))
    pos = sum(c.meta["packed"] for c in out)
    assert pos % kE4RingBytes == 0
    for kind in ("dense", "dense+L"):
        for ph in range(16):
            nfill = ((ph - pos) * 11) % 16   # 3 bytes per M word, 3 * 11 = 1 mod 16
            fill = Case(f"ring/filler/{kind}/before-obase%16={ph}", "ring", bg(nfill), kind="filler")
            pos += len(oracle.pack(fill.words))
            assert pos % 16 == ph
            name = f"ring/{kind}/obase%16={ph}/len{RING_DENSE}"
            words = np.concatenate([run_words(kind, RING_DENSE, _rng(name)), bg(3)])
            c = Case(name, "ring", words, kind=kind, start=0, length=RING_DENSE, obase=pos)
            pos += len(oracle.pack(c.words))
            out += [fill, c]
    return out


def _tiny(rng, n: int) -> np.ndarray:
    """n words of random classes (Z, M, D, L, a word with three zero bytes)."""
    w = dense(rng, n)
    for i, k in enumerate(rng.integers(0, 5, size=n)):
        if k == 0:
            w[i] = 0
        elif k == 1:
            w[i] = BG
        elif k == 3:
            w[i, rng.integers(0, 8)] = 0
        elif k == 4:
            w[i, rng.choice(8, size=3, replace=False)] = 0
    return w


LINES_PIECES = 600


def lines_cases():
    """Pieces of 1 to 3 words, several to a 16-byte output line; every fifth
    piece empty, and the first and the last."""
    rng = _rng("lines")
    out = []
    for i in range(LINES_PIECES):
        n = 0 if i % 5 == 0 or i == LINES_PIECES - 1 else int(rng.integers(1, 4))
        out.append(Case(f"lines/{i}/w{n}", "lines", _tiny(rng, n), kind="tiny"))
    return out


SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193,
         130, 330, 400)   # (the last three: 3, 6 and 7 steps -- every nsteps % 8 is present)


def sizes_cases():
    import step_model
    return [Case(f"sizes/rand/W{W}", "sizes", np.frombuffer(step_model.rand_piece(_rng("sizes", W), W), np.uint8),
                 kind="rand") for W in SIZES]


MANY = (kE4ScanBlock - 1, kE4ScanBlock, kE4ScanBlock + 1, 2 * kE4ScanBlock + 1)


def many_cases(n: int):
    """n pieces of 0 to 3 words."""
    rng = _rng("many", n)
    sizes = rng.integers(0, 4, size=n)
    return [Case(f"many{n}/{i}/w{int(s)}", "many", _tiny(rng, int(s)), kind="tiny") for i, s in enumerate(sizes)]


# ---- corpora -----------------------------------------------------------------------
PLANTED = ("step", "group", "zcap", "long", "count")   # one planted run each: walked and modelled on the CPU
CORPORA = PLANTED + ("ring", "lines", "sizes") + tuple(f"many{n}" for n in MANY)
MESSAGE_CORPORA = ("step", "count", "ring")             # grouped four segments to a message


def batch_arrays(cases):
    """-> (unpacked bytes uint8, seg_word_off uint64[n+1])."""
    data = np.concatenate([c.words for c in cases] + [np.zeros(0, np.uint8)])
    swo = np.concatenate([[0], np.cumsum([c.nwords for c in cases], dtype=np.uint64)]).astype(np.uint64)
    return data, swo


@lru_cache(maxsize=None)
def corpora() -> dict:
    """Every corpus, built once: {name: [Case]}; each is one batch."""
    check_pins()
    c = {"step": step_cases(), "group": group_cases(), "zcap": zcap_cases(), "long": long_cases(),
         "count": count_cases(), "ring": ring_cases(), "lines": lines_cases(), "sizes": sizes_cases()}
    for n in MANY:
        c[f"many{n}"] = many_cases(n)
    assert tuple(c) == CORPORA
    for name, cases in c.items():
        W = sum(x.nwords for x in cases)
        # (packed: the format's bound, 8 w + 2 ceil(w / 2) per piece)
        P = sum(8 * x.nwords + 2 * ((x.nwords + 1) // 2) for x in cases)
        assert 8 * W <= LIMIT_WORDS and P <= LIMIT_PACKED, (name, W, P)
    return c


def release():
    """Drop the built corpora; the test modules call it when they are done."""
    corpora.cache_clear()
