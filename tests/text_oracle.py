"""Oracle of the text validator (include/wsframe_amd_text.h), built on CPython's strict UTF-8
decoder (never its incremental decoder, which is quirky on partial input: it buffers ED A0 but
rejects E0 80). It keeps each connection's bytes so far in Python across batches and derives the
verdicts, first_bad and the exact state word from them. No GPU, no library of the project."""
import itertools

NA, VALID, INVALID = 0, 1, 2
NONE = 0xFFFFFFFF
ST_PENDING, ST_FAILED = 0x80000000, 0x40000000

# 0..3 bytes over {80, 90, A0}: that set completes every lead's restricted second-byte range
SUFFIXES = [bytes(s) for n in range(4) for s in itertools.product((0x80, 0x90, 0xA0), repeat=n)]


def complete_ok(b):
    try:
        bytes(b).decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def viable_literal(b):
    """b is a prefix of some well-formed string: the definition, 40 strict decodes"""
    b = bytes(b)
    return any(complete_ok(b + s) for s in SUFFIXES)


def tail_start(b):
    """the largest k with complete_ok(b[:k]) and len(b) - k <= 3, or None"""
    for k in range(len(b), max(len(b) - 3, 0) - 1, -1):
        if complete_ok(b[:k]):
            return k
    return None


def viable(b):
    """viable_literal, cheaply: b + s is well formed iff b[:k] is (k = tail_start) and b[k:] + s is,
    because a well-formed prefix ends on a sequence boundary (test_text_host checks the two agree)"""
    b = bytes(b)
    k = tail_start(b)
    return k is not None and any(complete_ok(b[k:] + s) for s in SUFFIXES)


def state_word(sofar):
    """the state an open text message with these bytes so far leaves"""
    if not viable(sofar):
        return ST_PENDING | ST_FAILED
    tail = bytes(sofar)[tail_start(sofar):]
    return ST_PENDING | len(tail) << 24 | int.from_bytes(tail, "little")


class TextConn:
    """One connection (one segment index over the batches). track=False: d_text_state is NULL,
    every batch stands alone."""

    def __init__(self, track=True):
        self.track = track
        self.pending = False       # the message left open is a text message
        self.sofar = b""           # ... and its bytes so far
        self.word = 0

    def batch(self, msgs):
        """msgs: the segment's listed messages in order, each (opcode, body, complete, continued,
        n_frames). Returns (verdicts, first_bad, state word or None when not tracked)."""
        verdicts, last_text, last_sofar = [], False, b""
        for opcode, body, complete, continued, n_frames in msgs:
            body = bytes(body)
            text = (self.track and self.pending) if continued else opcode == 1
            sofar = (self.sofar + body) if (continued and text) else body
            if text:
                ok = complete_ok(sofar) if complete else viable(sofar)
                verdicts.append(VALID if ok else INVALID)
            elif opcode == 8 and not continued and complete and n_frames == 1:
                verdicts.append(VALID if complete_ok(body[2:]) else INVALID)
            else:
                verdicts.append(NA)
            last_text, last_sofar = text, sofar
        if msgs and not msgs[-1][2]:                       # the last listed message is open
            self.pending = last_text
            self.sofar = last_sofar if last_text else b""
            self.word = state_word(last_sofar) if last_text else 0
        elif any(m[3] for m in msgs):                      # a continued message closed the pending one
            self.pending, self.sofar, self.word = False, b"", 0
        bad = [i for i, v in enumerate(verdicts) if v == INVALID]
        return verdicts, (bad[0] if bad else NONE), (self.word if self.track else None)
