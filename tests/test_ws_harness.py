"""The workspace harness of tests/ws_cases.py on numpy stand-ins for a library call: it passes a clean call and fails, naming
the kind of defect, a call that reads a workspace word before writing it, one that writes a byte behind its workspace, one that
leaves an output slot unwritten and one whose result depends on what the previous call left behind. No GPU: this is what shows
that the -m gpu tests built on the harness would fail on the bugs they exist for."""
import numpy as np
import pytest

import ws_cases as W

WS_BYTES = 1000            # not a multiple of 4 or 256: the band behind starts at an odd address
OUTS = [("scores", 64), ("ids", 128)]


def _clean(ws, scores, ids, n=16):
    """A well-behaved call: clears its counter, counts into it, writes every output slot."""
    cnt = ws[:4].view(np.uint32)
    cnt[0] = 0
    for k in range(n):
        ws[8 + k] = 3 * k + 1                      # written before read
        cnt[0] += 1
    scores[:] = 0
    scores[:n] = ws[8:8 + n]
    ids.view(np.int64)[:] = -1
    ids.view(np.int64)[:int(cnt[0])] = np.arange(int(cnt[0]))


def test_fills_are_the_four_patterns_in_order_benign_first():
    names = [f.name for f in W.fills()]
    assert names == ["0x00", "words=1", "random", "0xFF"]
    bufs = []
    for f in W.fills():
        b = np.full(37, 0x33, np.uint8)
        W.apply_fill(b, f)
        bufs.append(b)
    assert not bufs[0].any() and (bufs[3] == 0xFF).all()
    assert (bufs[1][:36].view("<u4") == 1).all() and bufs[1][36] == 1
    again = np.empty(37, np.uint8)
    W.apply_fill(again, W.RANDOM)
    assert np.array_equal(again, bufs[2]) and len(np.unique(bufs[2])) > 8          # seeded, and not a constant


def test_guarded_hands_out_exactly_the_bytes_asked_for_inside_two_bands():
    g = W.guarded(WS_BYTES, W.ALL_FF)
    assert g.interior.size == WS_BYTES and g.whole.size == WS_BYTES + 2 * W.GUARD
    assert g.interior.base is g.whole and (g.interior == 0xFF).all()
    assert (g.whole[:W.GUARD] == W.GUARD_BYTE).all() and (g.whole[W.GUARD + WS_BYTES:] == W.GUARD_BYTE).all()
    assert W.GUARD % 256 == 0 and W.GUARD_BYTE not in (0x00, 0x01, 0xFF)


def test_a_clean_call_passes_and_returns_the_first_run():
    got = W.run_independent(_clean, OUTS, WS_BYTES)
    assert got["scores"][:16].tolist() == [3 * k + 1 for k in range(16)] and not got["scores"][16:].any()
    assert got["ids"].view(np.int64).tolist() == list(range(16))
    same = W.run_after([_clean, lambda ws, s, i: _clean(ws, s, i, n=5)], _clean, OUTS, WS_BYTES, got)
    assert np.array_equal(same["ids"], got["ids"])


def test_a_read_before_write_of_a_workspace_word_fails():
    def call(ws, scores, ids):
        stale = int(ws[:4].view(np.uint32)[0])     # a counter nobody cleared
        _clean(ws, scores, ids)
        scores[20] = (stale + 1) & 0x7f
    with pytest.raises(W.WsFailure, match=r"fill words=1 differs from fill 0x00 in output 'scores' at byte offset 20") as e:
        W.run_independent(call, OUTS, WS_BYTES)
    assert e.value.kind == "workspace-dependent"


def test_one_byte_behind_the_workspace_fails():
    def call(ws, scores, ids):
        _clean(ws, scores, ids)
        ws.base[W.GUARD + ws.size] = 7             # the first byte behind the interior
    with pytest.raises(W.WsFailure, match=r"wrote behind its workspace of 1000 bytes: byte \+0 from the end") as e:
        W.run_independent(call, OUTS, WS_BYTES)
    assert e.value.kind == "guard-band"

    def before(ws, scores, ids):
        _clean(ws, scores, ids)
        ids.base[W.GUARD - 1] = 0                  # and one in front of an output
    with pytest.raises(W.WsFailure, match=r"wrote in front of output 'ids': byte -1 from the start") as e:
        W.run_independent(before, OUTS, WS_BYTES)
    assert e.value.kind == "guard-band"


def test_an_unwritten_output_slot_fails():
    def skips(ws, scores, ids):                    # pads the empty slots of the ids from slot 10 on: slot 9 is nobody's
        cnt = ws[:4].view(np.uint32)
        cnt[0] = 16
        scores[:] = 0
        v = ids.view(np.int64)
        v[:9] = np.arange(9)
        v[10:] = -1
    with pytest.raises(W.WsFailure, match=r"in output 'ids' at byte offset 72 .*never wrote the slot") as e:
        W.run_independent(skips, OUTS, WS_BYTES)
    assert e.value.kind == "unwritten-output"


def test_a_result_that_depends_on_the_previous_calls_leftovers_fails():
    """The select's protocol gone wrong: the call counts into a counter it expects the PREVIOUS call to have left at zero, and
    clears it only on its common path."""
    def call(ws, scores, ids, n=16, overflow=False):
        cnt = ws[4:8].view(np.uint32)
        if ws[0] != 0x5a:                           # first use of this workspace: the one memset
            cnt[0] = 0
            ws[0] = 0x5a
        cnt[0] += n
        scores[:] = 0
        scores[0] = int(cnt[0]) & 0xff
        ids.view(np.int64)[:] = -1
        if not overflow:                            # the path that forgets: the overflow fallback returns early
            cnt[0] = 0
    alone = W.run_after([], call, OUTS, WS_BYTES, {})
    assert alone["scores"][0] == 16
    ok = W.run_after([call, call], call, OUTS, WS_BYTES, {"scores": alone["scores"], "ids": alone["ids"]})
    assert ok["scores"][0] == 16
    with pytest.raises(W.WsFailure, match=r"after 2 earlier call\(s\) in the same workspace, output 'scores' differs .* byte offset 0") as e:
        W.run_after([call, lambda ws, s, i: call(ws, s, i, n=3, overflow=True)], call, OUTS, WS_BYTES,
                    {"scores": alone["scores"], "ids": alone["ids"]})
    assert e.value.kind == "leftover-dependent"
    # a window of a shared output: (byte offset, bytes)
    W.run_after([], call, OUTS, WS_BYTES, {"ids": (64, alone["ids"][64:])})
