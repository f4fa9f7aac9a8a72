"""The rules of tests/_encode_messages_at_model.py on hand-written cases, the
expected values written out here by hand (no GPU): exact fit, one byte short,
a slot past out_cap, a slot smaller than the table, saturating off + cap."""
import numpy as np

import _encode_messages_at_model as M

S = 0xA5
ONES = bytes([1] * 8)
# one segment of one word 0x0101010101010101: the table, ints (0, 1), is one
# word with byte 4 set and packs to tag 0x10 and that byte; the segment packs
# to tag 0xff, its 8 bytes and a literal-run count of 0
MSG = [ONES]
TABLE = bytes([0x10, 0x01])
SEG = bytes([0xff] + [1] * 8 + [0])
BODY = TABLE + SEG  # 12 bytes


def _exp(oracle, msgs, off, cap, out_cap, maxw=8, size=96):
    return M.expected(oracle, msgs, off, cap, out_cap, maxw, size, S)


def test_the_hand_packed_message(oracle):
    assert M.table_bytes(MSG) == bytes([0, 0, 0, 0, 1, 0, 0, 0])
    assert M.packed_pieces(oracle, MSG) == [TABLE, SEG]
    assert oracle.write_message(MSG) == BODY
    # a two-segment table has a pad half-word
    assert M.table_bytes([ONES, ONES + ONES]) == bytes([1, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0])


def test_exact_fit(oracle):
    e = _exp(oracle, [MSG], [7], [12], 64)
    assert e.status == [M.OK] and e.msg_len == [12] and e.piece_off == [7, 9]
    assert e.image[7:19].tobytes() == BODY
    assert (e.image[:7] == S).all() and (e.image[19:] == S).all() and e.care.all()


def test_one_byte_short(oracle):
    e = _exp(oracle, [MSG, MSG], [7, 40], [11, 12], 64)
    assert e.status == [M.ENOMEM, M.OK] and e.msg_len == [12, 12] and e.piece_off == [7, 9, 40, 42]
    assert (e.image[:40] == S).all() and e.image[40:52].tobytes() == BODY
    # the refused message's own slot is undefined, nothing else is
    assert not e.care[7:18].any() and e.care[:7].all() and e.care[18:].all()


def test_slot_past_out_cap(oracle):
    # the slot starts past out_cap: no byte of it may be stored
    e = _exp(oracle, [MSG], [70], [12], 64)
    assert e.status == [M.ENOMEM] and e.msg_len == [12] and e.care.all() and (e.image == S).all()
    # the slot ends one byte past out_cap although the message would fit below it
    e = _exp(oracle, [MSG], [40], [25], 64)
    assert e.status == [M.ENOMEM] and not e.care[40:64].any() and e.care[64:].all() and e.care[:40].all()
    # without capacities the slot runs to out_cap: 12 bytes fit exactly, 11 do not
    assert _exp(oracle, [MSG], [52], None, 64).status == [M.OK]
    e = _exp(oracle, [MSG], [53], None, 64)
    assert e.status == [M.ENOMEM] and not e.care[53:64].any() and e.care[64:].all()
    assert _exp(oracle, [MSG], [65], None, 64).status == [M.ENOMEM]


def test_slot_smaller_than_the_table(oracle):
    # a table that does not fit is not stored at all: the whole slot stays
    for cap in (0, 1):
        e = _exp(oracle, [MSG], [7], [cap], 64)
        assert e.status == [M.ENOMEM] and e.msg_len == [12] and e.care.all() and (e.image == S).all()
    # the table fits, the segment does not: the slot is undefined
    e = _exp(oracle, [MSG], [7], [2], 64)
    assert e.status == [M.ENOMEM] and not e.care[7:9].any() and e.care[9:].all()


def test_saturating_off_plus_cap(oracle):
    # off + cap wraps 2^64 to 8: taken as it stands the slot would be [16, 8);
    # saturated it passes out_cap, so the message is refused and only
    # [16, out_cap) is undefined
    cap = (1 << 64) - 8
    assert (16 + cap) & M.U64 == 8
    assert M.slot(16, cap, 64) == (True, 64)
    e = _exp(oracle, [MSG], [16], [cap], 64)
    assert e.status == [M.ENOMEM] and not e.care[16:64].any() and e.care[:16].all() and e.care[64:].all()
    # the largest capacity from the largest offset: the slot is empty
    assert M.slot(M.U64, M.U64, 64) == (True, 64)
    e = _exp(oracle, [MSG], [M.U64], [M.U64], 64)
    assert e.status == [M.ENOMEM] and e.care.all()


def test_segment_over_the_bound(oracle):
    e = _exp(oracle, [MSG, [ONES * 9], MSG], [0, 20, 60], [12, 30, 12], 80, maxw=8)
    assert e.status == [M.OK, M.EINVAL, M.OK] and e.defined == [True, False, True]
    assert e.msg_len == [12, None, 12] and not e.care[20:50].any() and e.care[50:].all()
    assert e.image[60:72].tobytes() == BODY
