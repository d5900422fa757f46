"""not-gpu: what acgpu_find_iter_batch / AhoCorasick.find_iter_batch decide on the host, before any device work."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from oracle import orc

INVALID_ARGUMENT = 22
OFF = np.array([0, 3, 6], dtype=np.uint64)


def call(a, skip=None):
    """the C entry point on b"foobar" in two segments, the argument named `skip` passed as NULL"""
    L = ac.load_library()
    hay = b"foobar"
    ci = _lib.CInput(C.cast(C.c_char_p(hay), C.c_void_p).value, len(hay), 0, len(hay), 0, 0, 0, 0, None)
    rec, buf, n_out = (C.c_uint64 * 3)(), (_lib.CMatch * 4)(), C.c_size_t()
    args = {"aut": a._h, "in": C.byref(ci), "offsets": C.c_void_p(OFF.ctypes.data), "n": 2, "overlapping": 0, "rec_offsets": rec,
            "out": buf, "cap": 4, "n_out": C.byref(n_out), "prof": None}
    if skip:
        args[skip] = None
    return L.acgpu_find_iter_batch(*args.values()), L.acgpu_last_error().decode()


@pytest.mark.parametrize("name", ["aut", "in", "offsets", "rec_offsets", "out", "n_out"])
def test_null_arguments_are_named(name):
    rc, why = call(ac.AhoCorasick.new([b"foo"]), skip=name)
    assert rc == INVALID_ARGUMENT and f"{name} is NULL" in why


def test_refused_before_device_work():
    a = ac.AhoCorasick.new([b"foo"])
    with pytest.raises(ac.MatchError) as e:   # StartKind::Unanchored: as the reference refuses every one of the searches
        a.find_iter_batch(b"foobar", OFF, anchored=True)
    assert e.value.kind == "InvalidInputAnchored"
    for mk in (ac.MatchKind.LeftmostFirst, ac.MatchKind.LeftmostLongest):
        with pytest.raises(ac.MatchError) as e:
            ac.AhoCorasick.builder().match_kind(mk).build([b"foo"]).find_iter_batch(b"foobar", OFF, overlapping=True)
        assert e.value.kind == "UnsupportedOverlapping"
    both = ac.AhoCorasick.builder().start_kind(ac.StartKind.Both).build([b"foo"])   # anchored overlapping: automaton.rs:409-419
    with pytest.raises(orc.OracleError, match="InvalidInputAnchored"):
        orc.Oracle([b"foo"], start_kind=0).find_overlapping_iter(b"foobar", span=(0, 3), anchored=True)
    with pytest.raises(ac.MatchError) as e:
        both.find_iter_batch(b"foobar", OFF, anchored=True, overlapping=True)
    assert e.value.kind == "InvalidInputAnchored"
    with pytest.raises(RuntimeError, match=r"offsets\[2\]"):
        a.find_iter_batch(b"foobar", np.array([0, 4, 3], dtype=np.uint64))
    for ovl in (False, True):   # zero segments: empty results
        records, rec_off = a.find_iter_batch(b"foobar", np.zeros(1, dtype=np.uint64), overlapping=ovl)
        assert len(records) == 0 and records.dtype == ac.MATCH_DTYPE and rec_off.tolist() == [0]
