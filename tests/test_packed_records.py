"""The record-level piece builder (tests/_packed_records.py) pinned against
the oracle, and the coverage the decoder seam corpora promise
(tests/test_gpu_decoder_seams.py runs them on the GPU).  No GPU needed.
"""
import numpy as np
import pytest

import _packed_records as R

# Bytes one GPU call may move: the limit holds for every corpus and for the
# concatenated stream, each of which is what one GPU test sends, not for
# their sum.  The sweeps as specified come to about 120 MiB packed and 450 MiB
# unpacked together (the first-window corpora alone to 49 MiB packed, the
# malformed end-of-piece variants to 19 MiB, the full-before-the-end variants
# to 29 MiB), so a limit on the sum could
# only be met by thinning them; test_corpus_totals prints the sum.
LIMIT_PACKED, LIMIT_WORDS = 64 << 20, 256 << 20


@pytest.fixture(scope="module")
def corpora():
    yield R.corpora()
    R.release()


def _oracle_batch(oracle, cases):
    packed, in_off, swo = R.batch_arrays(cases)
    return oracle.unpack_batch(packed, in_off, swo, threads=8)


def test_constants_are_the_sources():
    """Every geometry constant is read from its kernel source, as a literal
    or an expression of parsed constants; anything else raises instead of
    falling back to a remembered value."""
    assert set(R.CONST) == set(R._CONSTANTS) and all(v > 0 for v in R.CONST.values())
    assert R.kWin == 64 * R.kDecChunk and R.kD2Win == 64 * R.kD2Chunk
    assert R.kDecChkReach == R.kWin + 2064 and R.LONGEST == 2050
    assert R.TAILS == (0, 40, R.kDecChkReach - 8, 2 * R.kWin)
    assert R.WORD_SEAMS == sorted({R.kRound, 2 * R.kRound, R.kD2Round, 2 * R.kD2Round})
    src = """
    constexpr uint32_t kA = 48u, kB = 3;  // two declarators
    constexpr uint32_t kC = 64 * kA;
    #ifndef K_D
    #define K_D (kC / 2 + 1)
    #endif
    constexpr int kE = sizeof(int);
    """
    known = {}
    for name, want in (("kA", 48), ("kB", 3), ("kC", 3072), ("K_D", 1537)):
        known[name] = R.parse_constant(src, name, known)
        assert known[name] == want, name
    for name in ("kE", "kMissing"):
        with pytest.raises(AssertionError):
            R.parse_constant(src, name, known)


def test_fill_hits_every_length():
    for style in R.STYLES:
        for n in [0] + list(range(2, 400)) + [3071, 3072, 3583, 3584, 3585, 7168]:
            packed, words, index = R.build(R.fill(n, style))
            assert len(packed) == n, (style, n)
            assert index == R.parse_records(packed)
            if style != "z0pair" and n:
                assert R.built(R.fill(n, style)).canonical, (style, n)


@pytest.mark.parametrize("name", R.VALID)
def test_valid_cases_are_what_the_builder_says(oracle, corpora, name):
    """oracle.unpack of every valid case: OK, the whole piece consumed (the
    batch form reports anything else as ETRAILING), exactly the builder's
    words.  And oracle.pack of those words gives the built bytes exactly
    when the builder calls the case canonical."""
    cases = corpora[name]
    out, st = _oracle_batch(oracle, cases)
    bad = [c.name for c, s in zip(cases, st) if s != 0]
    assert not bad, bad[:8]
    assert out.tobytes() == b"".join(c.words for c in cases)
    _, _, swo = R.batch_arrays(cases)
    pk, off = oracle.pack_batch(out, swo, threads=8)
    wrong = [c.name for i, c in enumerate(cases)
             if (pk[int(off[i]):int(off[i + 1])].tobytes() == c.packed) != c.canonical]
    assert not wrong, wrong[:8]
    # one case through the single-piece entry point as well
    s, words, used = oracle.unpack(cases[0].packed, 8 * cases[0].nwords)
    assert (s, words, used) == (0, cases[0].words, len(cases[0].packed))


@pytest.fixture(scope="module")
def malformed_status(corpora):
    """{case name: the status name the builder predicts}, which the GPU
    tests' failure messages show next to the status they got."""
    return {c.name: c.expect for name in R.MALFORMED for c in corpora[name]}


@pytest.mark.parametrize("name", R.MALFORMED)
def test_malformed_cases_fail_as_predicted(oracle, corpora, malformed_status, name):
    """The status the builder predicts for each malformed case (cut short:
    ETRUNC; a word fewer: the last run overruns, or its last record is left
    unread; a word more: ETRUNC) is the oracle's."""
    cases = corpora[name]
    _, st = _oracle_batch(oracle, cases)
    wrong = [(c.name, malformed_status[c.name], R.STATUS[int(s)]) for c, s in zip(cases, st)
             if R.STATUS[int(s)] != malformed_status[c.name]]
    assert not wrong, wrong[:8]
    assert {"ETRUNC"} <= set(malformed_status.values())
    if name.startswith("endbad"):
        assert {c.expect for c in cases} == {"ETRUNC", "EOVERRUN", "ETRAILING"}
    if name.startswith("full/"):
        # full before the bytes end: the reference stops at the full point, so
        # never ETRUNC, whatever the tail ends in
        assert {c.expect for c in cases} == {"EOVERRUN", "ETRAILING"}


FULL_SEAMS = {
    "full/words-sparse": ({f"round{Rd}" for Rd in R.WORD_SEAMS}, R.WORD_PROBES),
    "full/words-mid": ({f"round{Rd}" for Rd in R.WORD_SEAMS}, R.WORD_PROBES),
    "full/first": ({f"win{R.kWin}"}, R.PROBES),
    "full/later": ({"winedge1|2", "winedge2|3"}, R.PROBES),
    "full/wrap": ({f"wrap{R.kMwWaves - 1}|{R.kMwWaves}", f"wrap{R.kMwWaves}|{R.kMwWaves + 1}"}, R.FULL_WRAP_KINDS),
}


def _window_of(starts, pos):
    return sum(s <= pos for s in starts) - 1


@pytest.mark.parametrize("name", list(R.FULL_SOURCES))
def test_full_point_variants_cover_their_sources(corpora, name):
    """Every full/* corpus against the bytes of its valid sources, read back
    with parse_records: each (seam, probe kind) of the source selection is
    there; the probe is a record of its kind at word o with t bytes behind
    it; every variant whose condition holds (full@probe: o > 0, full+1:
    nw > 1, full@end-1: nw > 2, full@end: t > 0) is present with the source's
    bytes and its word count, and cut by one byte when t >= 2; nothing else
    is.  Some /tailcut case loses its byte in a later window than the one it
    is full in, by the block map's windows and by the record index's."""
    src = R.full_sources(corpora, name)
    got = {c.name: c for c in corpora[name]}
    assert len(got) == len(corpora[name])
    seams, kinds = FULL_SEAMS[name]
    assert {(c.name.split("/")[0], c.kind) for c in src} == {(s, k) for s in seams for k in kinds}
    if name == "full/first":
        assert {c.name.split("/")[3] for c in src} == set(R.STYLES)
        assert {c.tag - R.kWin for c in src} == {-2, -1, 0, 1, 2} and {c.tail for c in src} == set(R.TAILS)
    if name == "full/wrap":
        assert all("/tag@+0/" in c.name for c in src)
    if name.startswith("full/words-"):
        # the full point R - d (+ 0, 1, nw - 1, nw) takes every phase of the kBlk-word block at every round edge
        for Rd in R.WORD_SEAMS:
            full = {c.nwords - Rd for c in corpora[name] if c.name.startswith(f"round{Rd}/")}
            assert set(range(-8, 2)) <= full, Rd
    want, later = set(), {R.kWin: 0, R.kD2Win: 0}
    for c in src:
        idx = R.parse_records(c.packed)
        i = next(i for i, (p, _, _) in enumerate(idx) if p == c.tag)
        o, kind = idx[i][1], idx[i][2]
        nw = (idx[i + 1][1] if i + 1 < len(idx) else c.nwords) - o
        t = len(c.packed) - (idx[i + 1][0] if i + 1 < len(idx) else len(c.packed))
        assert (kind, o, t) == (c.kind, c.word, c.tail), c.name
        variants = {"full@probe": (o, o > 0), "full+1": (o + 1, nw > 1), "full@end-1": (o + nw - 1, nw > 2),
                    "full@end": (o + nw, t > 0)}
        assert set(variants) == set(R.FULL_VARIANTS)
        for v, (nwords, holds) in variants.items():
            for cut in ("", "/tailcut"):
                full = f"{c.name}/{v}{cut}"
                if not (holds and (not cut or t >= 2)):
                    assert full not in got, full
                    continue
                want.add(full)
                x = got[full]
                assert x.nwords == nwords and x.words is None and not x.canonical, full
                assert x.packed == (c.packed[:-1] if cut else c.packed), full
                if not cut:
                    continue
                # the record that fills (or overruns) the piece, and the record the cut lands in
                j = max(k for k, (_, w, _) in enumerate(idx) if w <= nwords - 1)
                for win, cap in ((R.kWin, None), (R.kD2Win, R.kD2NI)):
                    starts = R.window_starts(idx, len(c.packed), win, cap)
                    later[win] += _window_of(starts, idx[-1][0]) > _window_of(starts, idx[j][0])
    assert want == set(got)
    print(f"\n{name}: {len(src)} sources, {len(got)} cases; /tailcut cases cut in a later window than they are "
          f"full in: {later[R.kWin]} (block map), {later[R.kD2Win]} (record index)")
    assert later[R.kWin] > 0 and later[R.kD2Win] > 0


def test_every_named_seam_is_present(corpora):
    names = {c.name for cs in corpora.values() for c in cs}
    n = 0
    for style in R.STYLES:
        seams = [R.kD2Win, R.kWin] + ([2 * R.kD2NI] if style in ("mid", "z0pair") else [])
        for S in seams:
            for kind in R.PROBES:
                for off in range(-R.kDecChunk - 4, 19):
                    assert any(f"win{S}/{kind}/tag@{off:+d}/{style}/tail{t}" in names for t in R.TAILS)
                    n += 1
        tails = {c.name.rsplit("/tail", 1)[1] for c in corpora[f"first/{style}"] if "/tail" in c.name}
        assert tails == {str(t) for t in R.TAILS}
    for w in (1, 2):
        for kind in R.PROBES:
            for off in range(-2, 3):
                assert f"winedge{w}|{w + 1}/{kind}/tag@{off:+d}/dense" in names
                assert f"wrap{w + R.kMwWaves - 2}|{w + R.kMwWaves - 1}/{kind}/tag@{off:+d}/dense" in names
    for style in ("sparse", "mid"):
        for Rd in (1280, 2560, 2048, 4096):
            assert Rd in R.WORD_SEAMS
            for kind in R.WORD_PROBES:
                for d in list(range(0, 9)) + [-1]:
                    assert f"round{Rd}/{kind}/word@{-d:+d}/{style}" in names
    for kind in R.PROBES:
        for d in range(-17, 18):
            for style in ("dense", "mid"):
                for v in ("", "/cut1", "/words-1", "/words+1"):
                    assert f"end/{kind}/reach{d:+d}/{style}{v}" in names
    for cnt in (1023, 1024, 1025):
        for kind in ("Z255", "F255"):
            assert f"reccap{R.kD2NI}/{kind}/records{cnt}/mid" in names
    for cnt in (127, 128, 129):
        assert f"sermax{R.kDecSerMax}/F2/records{cnt}/dense/0" in names
    # full before the bytes end (test_full_point_variants_cover_their_sources has the whole list)
    for v in R.FULL_VARIANTS:
        for cut in ("", "/tailcut"):
            for Rd in (1280, 2560, 2048, 4096):
                for style in ("sparse", "mid"):
                    assert f"round{Rd}/Z255/word@-3/{style}/{v}{cut}" in names
                    assert f"round{Rd}/F255/word@+0/{style}/tail{2 * R.kWin}/{v}{cut}" in names
            for w in (1, 2):
                assert f"winedge{w}|{w + 1}/F255/tag@-1/dense/{v}{cut}" in names
                assert f"wrap{w + R.kMwWaves - 2}|{w + R.kMwWaves - 1}/Z255/tag@+0/dense/{v}{cut}" in names
    for style in R.STYLES:
        assert any(f"win{R.kWin}/F255/tag@+0/{style}/tail{t}/full+1" in names for t in R.TAILS)
    print(f"\n{n} first-window (seam, kind, offset, style) points; {len(names)} named cases")


def test_probes_stand_where_the_names_say(corpora):
    """Read back from the bytes alone (parse_records), with the placement
    rule: the probe of every later-window, wave-wrap, word-seam, record-count
    and end-of-piece case is a record of its kind at its place."""
    for name in ("later/dense", "wrap/dense"):
        for c in corpora[name]:
            idx = R.parse_records(c.packed)
            starts = R.window_starts(idx, len(c.packed), R.kWin)
            w = int(c.name.split("/")[0].split("|")[1])
            off = int(c.name.split("tag@")[1].split("/")[0])
            assert (c.tag, c.kind) in {(p, k) for p, _, k in idx}, c.name
            assert c.tag == starts[w - 1] + R.kWin + off, c.name
            assert len(starts) >= (4 if name == "later/dense" else R.kMwWaves + 2), c.name
            assert 6 * 1024 <= len(c.packed) < 384 * 1024
    for style in ("sparse", "mid"):
        for c in corpora[f"words/{style}"]:
            idx = R.parse_records(c.packed)
            Rd = int(c.name.split("/")[0][5:])
            d = int(c.name.split("word@")[1].split("/")[0])
            assert (c.tag, Rd + d, c.kind) in idx, c.name
            assert c.tag < R.kD2Win and len(R.window_starts(idx[: idx.index((c.tag, Rd + d, c.kind)) + 1],
                                                            c.tag + 1, R.kD2Win, R.kD2NI)) == 1, c.name
    for c in corpora["count/mid"]:
        idx = R.parse_records(c.packed)
        n = int(c.name.split("records")[1].split("/")[0])
        assert idx[n][0] == c.tag == 2 * n and idx[n][2] == c.kind and all(k == "T1" for _, _, k in idx[:n])
    for c in corpora["count/dense"]:
        idx = R.parse_records(c.packed)
        starts = R.window_starts(idx, len(c.packed), R.kWin)
        n = int(c.name.split("records")[1].split("/")[0])
        inwin = [p for p, _, _ in idx if starts[1] <= p < starts[1] + R.kWin]
        assert starts[1] == c.tag and len(inwin) == n and len(c.packed) - starts[1] >= R.kDecChkReach, c.name
    for style in ("dense", "mid"):
        for c in corpora[f"end/{style}"]:
            idx = R.parse_records(c.packed)
            starts = R.window_starts(idx, len(c.packed), R.kWin)
            d = int(c.name.split("reach")[1].split("/")[0])
            assert idx[-1][0] == c.tag and idx[-1][2] == c.kind, c.name
            assert len(c.packed) - starts[1] == R.kDecChkReach + d, c.name
            if c.tag >= starts[1] + R.kWin:
                assert starts[-2] == starts[1], c.name


def test_batches_go_where_the_gate_sends_them(corpora):
    """dec_gate_kernel's thresholds (15 % / 80 % of the words' bytes) over
    each corpus as one batch: sparse to the record index, mid to the block
    map, dense to the dense form."""
    for name, want in R.GATE.items():
        assert R.gate_of(corpora[name]) == want, name
    # with the record index forced, a mid window holds more records than its cap
    some = corpora["first/mid"][::16]
    over = [c for c in some if sum(p < R.kD2Win for p, _, _ in R.parse_records(c.packed)) > R.kD2NI]
    assert len(over) > len(some) // 2


def test_first_window_batches_take_every_load_phase(corpora):
    for style in R.STYLES:
        assert R.in_off_phases(corpora[f"first/{style}"]) == set(range(16)), style


def test_stream_covers_block_and_group_edges(corpora):
    """The concatenated stream of the first-window and non-canonical pieces:
    each probe kind's tag covers every residue of [kSsBlock - 12, kSsBlock + 2]
    mod kSsBlock, and an F255 probe starts in the last block of a group."""
    cases = R.stream_of([c for s in R.STYLES for c in corpora[f"first/{s}"]] + corpora["noncanon"])
    res, last = R.stream_coverage(cases)
    print("\nresidues covered per probe kind:", {k: len(v) for k, v in sorted(res.items())},
          "; F255 probes in a group's last block:", last)
    assert last > 0
    for kind in R.PROBES:
        assert set(R.STREAM_RESIDUES) <= res[kind], kind
    P, U = sum(len(c.packed) for c in cases), 8 * sum(c.nwords for c in cases)
    print(f"stream: {len(cases)} pieces, {P / 2**20:.1f} MiB packed, {U / 2**20:.1f} MiB unpacked")
    assert P + 3000 <= LIMIT_PACKED and U <= LIMIT_WORDS


def test_corpus_totals(corpora):
    """No corpus, which is what one GPU call moves, passes 64 MiB packed or
    256 MiB unpacked; the totals are printed."""
    tp = tu = 0
    print()
    for name, cases in corpora.items():
        P, U = sum(len(c.packed) for c in cases), 8 * sum(c.nwords for c in cases)
        print(f"{name:14s} {len(cases):5d} cases {P / 2**20:7.2f} MiB packed {U / 2**20:7.2f} MiB unpacked "
              f"-> {R.gate_of(cases)}")
        assert P <= LIMIT_PACKED and U <= LIMIT_WORDS, name
        assert len({c.name for c in cases}) == len(cases), name
        tp, tu = tp + P, tu + U
    print(f"all corpora: {tp / 2**20:.1f} MiB packed, {tu / 2**20:.1f} MiB unpacked")
    assert len(corpora["rounds/sparse"][0].packed) == R.kWin and corpora["rounds/sparse"][0].nwords == 128 * R.kWin
