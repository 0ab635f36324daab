"""CPU: the Merlin v1.0 transcript behind the C ABI (sbn_transcript_*) against tests/transcript_model.py, byte for byte.

No GPU: the transcript entry points need no context.  The model is checked first, against the known answer of the Merlin
specification's test protocol and (its Keccak-f) against hashlib's SHA3-256."""
import ctypes as C
import hashlib

import pytest

import transcript_model as tm

R = tm.R_MOD
KAT = "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"


# ---- the model itself ---------------------------------------------------------------------------------------------------------

def test_model_keccak_f_vs_sha3():
    st = bytearray(200)
    st[0] = 0x06
    st[135] ^= 0x80                      # SHA3-256 of the empty message: one padded block
    assert bytes(tm.keccak_f1600(st)[:32]) == hashlib.sha3_256(b"").digest()


def test_model_known_answer():
    t = tm.Transcript(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32).hex() == KAT


def test_model_round_costs_two_permutations_behind_a_challenge():
    t = tm.Transcript(b"x")
    tm.sumcheck_round_step(t, 5, 1, 2, 3)
    assert t.s.pos == 64                 # every round ends behind the PRF's 64 bytes ...
    p0 = t.permutations
    tm.sumcheck_round_step(t, 5, 1, 2, 3)
    assert t.permutations - p0 == 2 and t.s.pos == 64      # ... so every later round is two permutations


# ---- the library against the model ----------------------------------------------------------------------------------------------

def _pair(sbn, label):
    return sbn.Transcript(label), tm.Transcript(label)


def _same(a, m):
    assert a.state() == m.state()


def test_known_answer(sbn):
    t = sbn.Transcript(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32).hex() == KAT


@pytest.mark.parametrize("n", [0, 1, 165, 166, 167, 1000])
def test_message_lengths(sbn, n):
    a, m = _pair(sbn, b"lengths")
    _same(a, m)
    msg = bytes((7 * i + n) & 0xff for i in range(n))
    a.append_message(b"m", msg); m.append_message(b"m", msg)
    _same(a, m)
    assert a.challenge_bytes(b"c", 32) == m.challenge_bytes(b"c", 32)
    _same(a, m)


@pytest.mark.parametrize("n", [1, 32, 64, 166, 400])
def test_challenge_lengths(sbn, n):
    a, m = _pair(sbn, b"challenges")
    a.append_message(b"seed", b"abc"); m.append_message(b"seed", b"abc")
    for _ in range(2):
        assert a.challenge_bytes(b"ch", n) == m.challenge_bytes(b"ch", n)
        _same(a, m)


def _at_phase(sbn, pos):
    """a library transcript and the model, both at STROBE position `pos` (reached by a filler message of the right length)"""
    a, m = _pair(sbn, b"phase")
    # append_message moves pos by 2 + len(label) + 4 + 2 + len(msg) modulo the rate
    k = (pos - m.s.pos - 9) % tm.RATE
    fill = bytes(range(k))
    a.append_message(b"f", fill); m.append_message(b"f", fill)
    assert m.s.pos == pos
    return a, m


def _round_ops(t, co):
    t.append_message(b"poly", b"UniPoly_begin")
    for c in co:
        t.append_message(b"coeff", c)
    t.append_message(b"poly", b"UniPoly_end")


def test_every_start_phase_of_a_sumcheck_round(sbn):
    co = [((0x1234567 << 200) * (k + 1) % R).to_bytes(32, "little") for k in range(4)]
    for pos in range(tm.RATE):
        a, m = _at_phase(sbn, pos)
        _same(a, m)
        _round_ops(a, co); _round_ops(m, co)
        _same(a, m)
        got = a.challenge_scalar(b"challenge_nextround")
        assert int.from_bytes(got, "little") == m.challenge_scalar(b"challenge_nextround"), pos
        _same(a, m)


def test_clone_is_independent(sbn):
    a, m = _pair(sbn, b"clone")
    b = a.clone()
    before = a.state()
    b.append_message(b"x", b"only in the clone")
    assert a.state() == before and b.state() != before
    m2 = m.clone(); m2.append_message(b"x", b"only in the clone")
    _same(b, m2)
    a.append_message(b"x", b"only in the clone")
    assert a.state() == b.state()
    b.free()
    assert a.challenge_bytes(b"c", 16) == m2.challenge_bytes(b"c", 16)


def test_state_round_trip(sbn):
    a, m = _at_phase(sbn, 100)
    b = sbn.Transcript.from_state(a.state())
    assert b.state() == a.state()
    for t in (a, b, m):
        t.append_message(b"after", b"the record")
    assert a.challenge_bytes(b"c", 200) == b.challenge_bytes(b"c", 200) == m.challenge_bytes(b"c", 200)
    assert a.state() == b.state() == m.state()


def test_challenge_scalar_reduces_64_bytes(sbn):
    a, m = _pair(sbn, b"scalars")
    for k in range(8):
        b64 = a.clone().challenge_bytes(b"s", 64)
        got = a.challenge_scalar(b"s")
        assert int.from_bytes(got, "little") == int.from_bytes(b64, "little") % R == m.challenge_scalar(b"s")
        assert int.from_bytes(got, "little") < R


def test_wide_reduction_extremes(sbn, ol):
    cases = [0, (1 << 512) - 1, R, R - 1, R << 256, (R << 256) - 1, (R - 1) << 256, 1 << 256, (1 << 256) - 1, R * R, 5 * R + 3]
    for v in cases:
        b64 = v.to_bytes(64, "little")
        got = sbn.fr_from_wide(b64)
        assert int.from_bytes(got, "little") == v % R, hex(v)
        assert got == ol.fr_from_wide(b64)


def test_argument_errors_leave_the_transcript_unchanged(sbn):
    L = sbn.lib()
    t = sbn.Transcript(b"errors")
    before = t.state()
    out = (C.c_uint8 * 32)()
    inval = -1
    assert L.sbn_transcript_append_message(t.h, None, C.c_size_t(3), b"abc", C.c_size_t(3)) == inval
    assert L.sbn_transcript_append_message(t.h, b"l", C.c_size_t(1), None, C.c_size_t(3)) == inval
    assert L.sbn_transcript_append_message(None, b"l", C.c_size_t(1), b"abc", C.c_size_t(3)) == inval
    assert L.sbn_transcript_challenge_bytes(t.h, b"l", C.c_size_t(1), None, C.c_size_t(8)) == inval
    assert L.sbn_transcript_challenge_bytes(t.h, None, C.c_size_t(1), out, C.c_size_t(8)) == inval
    assert L.sbn_transcript_challenge_scalar(t.h, b"l", C.c_size_t(1), None) == inval
    assert L.sbn_transcript_state(t.h, None) == inval
    assert L.sbn_transcript_state(None, out) == inval
    h = C.c_void_p()
    assert L.sbn_transcript_new(None, C.c_size_t(4), C.byref(h)) == inval
    assert L.sbn_transcript_new(b"x", C.c_size_t(1), None) == inval
    assert L.sbn_transcript_clone(None, C.byref(h)) == inval
    assert L.sbn_transcript_from_state(None, C.byref(h)) == inval
    for bad in (before[:200] + bytes([166, 0, 0]), before[:200] + bytes([0, 167, 0]), before[:200] + bytes([0, 0, 0x40])):
        assert L.sbn_transcript_from_state(bad, C.byref(h)) == inval
    assert h.value is None
    assert L.sbn_fr_from_wide(None, out) == inval
    assert t.state() == before
    # empty label and empty message are valid, with or without a pointer
    m = tm.Transcript(b"errors")
    assert L.sbn_transcript_append_message(t.h, None, C.c_size_t(0), None, C.c_size_t(0)) == 0
    m.append_message(b"", b"")
    assert t.state() == m.state()
    L.sbn_transcript_free(None)
