"""The guarded arena of tests/guarded.py, on CPU tensors: the layout to the byte, a clean call, and the mutants check() has to catch
and name -- a stray byte on either side of a buffer, the arena's very last byte, a changed input, and stores whose bytes are not the
fill (zero, a canonical NaN)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded as G

SIZES = [0, 1, 3, 4, 257]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arena(capacity=None):
    """Buffers of SIZES bytes: in, out, inout, scratch, in."""
    a = G.Arena("cpu", capacity or G.capacity_for(SIZES))
    roles = ["in", "out", "inout", "scratch", "in"]
    for k, (nb, role) in enumerate(zip(SIZES, roles)):
        init = np.arange(nb, dtype=np.uint8) if role in ("in", "inout") else None
        a.take("b%d" % k, nb, role, init)
    return a


def test_guard_condition():
    assert G.GUARD == 64 * 1024 and G.GUARD >= 256 * 22 * 8 == G.WIDEST_TILE_BYTES


def test_layout_bases_and_adjacent_guards():
    bases, total = G.layout(SIZES)
    a = arena()
    assert a.capacity == G.round_up(total)
    assert [b.base for b in a.bufs] == bases
    prev_end = 0
    for b, nb in zip(a.bufs, SIZES):
        assert b.base % 256 == 0 and b.nbytes == nb and b.ptr == a.mem.data_ptr() + b.base and b.ptr % 256 == 0
        assert b.base - prev_end >= (2 * G.GUARD if prev_end else G.GUARD)            # a whole guard on each side of every buffer
        prev_end = b.base + nb
    assert a.capacity - prev_end >= G.GUARD
    # guards adjacent to the byte: everything outside the buffers is the fill, the byte before a base and the byte at base + nbytes included
    inside = np.zeros(a.capacity, bool)
    for b in a.bufs:
        inside[b.base:b.base + b.nbytes] = True
    mem = a.mem.numpy()
    assert (mem[~inside] == 0xFF).all()
    regions = a._regions()
    covered = np.zeros(a.capacity, int)
    for b, side, lo, hi, origin in regions:
        covered[lo:hi] += 1
        assert origin == (b.base if side == "before" else b.base + b.nbytes)
        assert (hi == b.base) if side == "before" else (lo == b.base + b.nbytes)      # no rounding of nbytes in between
        assert hi - lo >= G.GUARD
    assert ((covered == 1) == ~inside).all() and (covered[inside] == 0).all()
    # fill and inits
    assert a["b1"].bytes() == b"\xff" and a["b3"].bytes() == b"\xff" * 4
    assert a["b2"].bytes() == bytes(range(3)) and a["b4"].bytes() == bytes(np.arange(257, dtype=np.uint8))
    assert a["b3"].view(__import__("torch").float32).numel() == 1


def test_clean_call_passes(capsys):
    a = arena()
    a["b1"]._t.fill_(7)          # what a call does: it writes its outputs, its scratch and its in-out buffers
    a["b2"]._t.fill_(9)
    a["b3"]._t.zero_()
    a.check("clean")
    assert "GUARD clean: 5 buffers, 265 bytes" in capsys.readouterr().out and a.findings() == []


def _caught(a, expect):
    assert a.findings() == [expect], a.findings()
    with pytest.raises(G.GuardError) as e:
        a.check("mutant")
    return str(e.value)


def test_one_byte_past_the_end():
    a = arena()
    b = a["b4"]
    a.mem[b.base + b.nbytes] = 0
    msg = _caught(a, ("b4", "after", 0, 0, 1))
    assert "guard after b4: 1 bytes changed, offsets 0..0 past the end" in msg
    a = arena()
    b = a["b2"]                                   # 3 bytes: the guard starts at base + 3, not at base + 4
    a.mem[b.base + 3] = 1
    _caught(a, ("b2", "after", 0, 0, 1))
    a = arena()                                   # an empty buffer: base itself is the guard after it
    a.mem[a["b0"].base] = 1
    _caught(a, ("b0", "after", 0, 0, 1))


def test_one_byte_before_the_base():
    a = arena()
    a.mem[a["b3"].base - 1] = 0
    msg = _caught(a, ("b3", "before", -1, -1, 1))
    assert "guard before b3: 1 bytes changed, offsets -1..-1 from the base" in msg


def test_last_byte_of_the_last_guard():
    a = arena()
    a.mem[a.capacity - 1] = 0x7F
    b = a["b4"]
    off = a.capacity - 1 - (b.base + b.nbytes)
    _caught(a, ("b4", "after", off, off, 1))
    a = arena()                                   # and the first byte of the first
    a.mem[0] = 0
    _caught(a, ("b0", "before", -a["b0"].base, -a["b0"].base, 1))


def test_one_byte_of_an_input():
    a = arena()
    a["b4"]._t[200] = 0xEE
    msg = _caught(a, ("b4", "input", 200, 200, 1))
    assert "input b4: 1 bytes changed, offsets 200..200" in msg
    a = arena()                                   # an in-out buffer may change
    a["b2"]._t[1] = 0xEE
    a.check("inout")


@pytest.mark.parametrize("word", [0x00000000, 0x7FC00000])
def test_stores_of_zero_and_of_a_canonical_nan(word):
    """A float store of 0.0 and one of the canonical NaN (bytes 00 00 C0 7F) each change all four guard bytes: the fill is a NaN too,
    but no NaN a kernel computes."""
    a = arena()
    b = a["b3"]
    a.mem[b.base + b.nbytes:b.base + b.nbytes + 4] = __import__("torch").from_numpy(np.array([word], dtype="<u4").view(np.uint8).copy())
    changed = [k for k, v in enumerate(np.array([word], dtype="<u4").view(np.uint8)) if v != 0xFF]
    assert len(changed) == 4
    _caught(a, ("b3", "after", changed[0], changed[-1], len(changed)))


def test_several_findings_and_refused_calls():
    a = arena()
    a.mem[a["b1"].base - 2:a["b1"].base + 3] = 0          # two before, the byte itself, two past
    assert a.findings() == [("b1", "before", -2, -1, 2), ("b1", "after", 0, 1, 2)]
    assert a.findings(untouched=True) == [("b1", "before", -2, -1, 2), ("b1", "after", 0, 1, 2), ("b1", "written", 0, 0, 1)]
    a = arena()
    a.check("refused", untouched=True)
    a["b3"]._t[2] = 0
    a["b2"]._t[0] = 5
    assert a.findings(untouched=True) == [("b2", "written", 0, 0, 1), ("b3", "written", 2, 2, 1)] and a.findings() == []


def test_plain_allocator_and_output_comparison():
    a, p = arena(), G.Plain("cpu")
    for b in a.bufs:
        p.take(b.name, b.nbytes, b.role, a._init.get(b.name))
    assert G.differing_outputs(a, p) == []
    p["b3"]._t[0] = 0            # scratch: not compared
    assert G.differing_outputs(a, p) == []
    p["b1"]._t[0] = 0
    assert G.differing_outputs(a, p) == ["b1"]
    with pytest.raises(AssertionError):
        a.take("b1", 4, "out")                                   # a name twice
    with pytest.raises(AssertionError):
        G.Arena("cpu", G.capacity_for([8])).take("x", 8 + G.ALIGN, "out")      # past the capacity
    with pytest.raises(AssertionError):
        G.Arena("cpu", G.capacity_for([8])).take("x", 8, "in", np.zeros(7, np.uint8))


def test_imports_without_torch_cuda():
    """The layout arithmetic needs no torch at all, and the test module's case tables no GPU."""
    code = ("import sys; sys.path.insert(0, %r); sys.modules['torch'] = None; import guarded as G; "
            "b, t = G.layout([0, 1, 257]); assert b[0] == G.GUARD and b[1] == 3 * G.GUARD and t == b[2] + 257 + G.GUARD; print('ok')"
            % os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
