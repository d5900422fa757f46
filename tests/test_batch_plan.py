"""not-gpu: which stepper acgpu_find_batch walks with (plan_batch, aho-corasick_amd/csrc/host/engine_plan.hpp) as a table over
real automata, and the errors of the call that are decided on the host, before any device work."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from oracle import orc

ROWS, DFA, CNFA = 3, 1, 2
INVALID_ARGUMENT = 22


@pytest.mark.parametrize("pats,kind,batch_rows,want", [
    ([b"app", b"append", b"ndag"], ac.AhoCorasickKind.DFA, 1, ROWS),
    ([b"app", b"append", b"ndag"], ac.AhoCorasickKind.DFA, 0, DFA),              # the variant
    (orc.gen_patterns(1000, seed=0xAC01), ac.AhoCorasickKind.DFA, 1, DFA),       # too large for the image
    ([b"app", b"append", b"ndag"], ac.AhoCorasickKind.ContiguousNFA, 1, CNFA),   # no DFA at all
])
def test_batch_plan_table(pats, kind, batch_rows, want):
    t = ac.AhoCorasick.builder().kind(kind).build(pats).tables()
    has_dfa = kind == ac.AhoCorasickKind.DFA
    out = (C.c_uint32 * 4)()
    facts = (C.c_uint64 * 4)(int(has_dfa), t.dfa_state_len, t.alphabet_len if has_dfa else 0, batch_rows)
    assert ac.load_test_hooks().acgpu_test_batch_plan(None, facts, out) == 0
    assert out[0] == want
    assert out[1] == ac.AhoCorasick.BATCH_TILE_BYTES
    # the image takes what 160 KiB of LDS leave beside four staging tiles and the class map, as u16 entries
    assert out[3] == (160 * 1024 - 4 * out[1] - 256) // 2
    if has_dfa:
        assert (want == ROWS) == (bool(batch_rows) and t.dfa_state_len * t.alphabet_len <= out[3])


def call(a, hay, offsets, n, out=True, anchored=0):
    L = ac.load_library()
    ci = _lib.CInput(C.cast(C.c_char_p(hay), C.c_void_p).value, len(hay), 0, len(hay), anchored, 0, 0, 0, None)
    off = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
    buf = (_lib.CMatch * max(n, 1))() if out else None
    rc = L.acgpu_find_batch(a._h, C.byref(ci), None if off is None else C.c_void_p(off.ctypes.data), n, buf, None)
    return rc, L.acgpu_last_error().decode()


def test_host_side_errors():
    a = ac.AhoCorasick.new([b"foo"])
    rc, why = call(a, b"foobar", None, 2)
    assert rc == INVALID_ARGUMENT and "offsets is NULL" in why
    rc, why = call(a, b"foobar", [0, 3, 6], 2, out=False)
    assert rc == INVALID_ARGUMENT and "out is NULL" in why
    rc, why = call(a, b"foobar", [0, 4, 3], 2)
    assert rc == INVALID_ARGUMENT and "offsets[2]" in why
    rc, why = call(a, b"foobar", [0, 3, 7], 2)
    assert rc == INVALID_ARGUMENT and "haystack_len" in why
    assert call(a, b"foobar", None, 0, out=False)[0] == 0   # an empty batch: OK, whatever else is passed
    assert len(a.find_batch(b"foobar", np.zeros(0, dtype=np.uint64))) == 0
    with pytest.raises(ac.MatchError) as e:   # StartKind::Unanchored: as the reference refuses every one of the searches
        a.find_batch(b"foobar", np.array([0, 3, 6], dtype=np.uint64), anchored=True)
    assert e.value.kind == "InvalidInputAnchored"
    assert ac.NO_MATCH == 0xFFFFFFFF
