"""Long-form synthesis, the parts that need no GPU: the tests' float64 reference of zvx_trim_bounds against the silence trimmer the
project ships, the sentence splitter, and header / binding agreement of the two new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import join_ref as J
from zerovox_amd import _lib
from zerovox_amd.longform import PAUSES_MS, split_sentences
from zerovox_amd.mels import trim_silence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(2048, 512), (1024, 256), (400, 160)]
TOP_DB = [25, 40, 60]


@pytest.mark.parametrize("seed", range(8))
def test_bounds_reference_makes_the_decisions_of_trim_silence(seed):
    """ties include/zvx.h's definition (powers in double, p > pmax k) to mels.trim_silence (RMS in f32, dB compare) on the GPU tests' rows"""
    trimmed = 0
    for frame, hop in FRAMES:
        for top_db in TOP_DB:
            for x in J.make_rows(seed):
                begin, end, worst = J.bounds_ref(x, frame, hop, top_db, keep=0)
                assert worst > 1e-6, (frame, hop, top_db, len(x), worst)           # no frame anywhere near the threshold: both must agree
                got = trim_silence(x, top_db=top_db, frame_length=frame, hop_length=hop)
                assert np.array_equal(got, x[begin:end]), (frame, hop, top_db, len(x), begin, end, len(got))
                trimmed += (frame, hop, top_db) == (2048, 512, 40) and (begin > 0 or end < len(x))
    assert trimmed >= 3, trimmed                                                   # the rows do exercise the trimmer


def test_reference_edge_rules():
    x = (np.random.default_rng(1).standard_normal(6000) * 0.1).astype(np.float32)
    x[:2500] = 0
    assert J.bounds_ref(x, top_db=0.0)[:2] == (0, 6000) and J.bounds_ref(x, top_db=-3.0)[:2] == (0, 6000)
    assert J.bounds_ref(x[:2047])[:2] == (0, 2047) and J.bounds_ref(x[:0])[:2] == (0, 0)
    assert J.bounds_ref(np.zeros(5000, np.float32))[:2] == (0, 5000)
    b0, e0, _ = J.bounds_ref(x, keep=0)
    b1, e1, _ = J.bounds_ref(x, keep=300)
    assert b0 > 0 and b1 == b0 - 300 and e1 == e0 == 6000                          # keep is clamped to the row
    seg = J.segment_ref(x, 3000, 3007, 5000)                                       # F = m // 2 = 3: the middle sample keeps its bits
    g = np.array([1, 3, 5], np.float32) / np.float32(6)
    assert np.array_equal(seg[:3], x[3000:3003] * g) and seg[3] == x[3003] and np.array_equal(seg[4:], x[3004:3007] * g[::-1])
    out, pos, begin, ln = J.join_ref([x[3000:3010], x[:0], x[3000:3004]], gaps=[2, 3, 1], top_db=0.0)
    assert list(pos) == [0, 12, 15] and list(ln) == [10, 0, 4] and len(out) == 20 and not out[10:12].any() and not out[19:].any()
    assert np.array_equal(J.pcm16(np.array([1.5, -1.5, 0.5, -0.00001], np.float32)), np.array([32767, -32768, 16380, 0], np.int16))


def test_split_sentences_closing_classes():
    got = split_sentences("Hello there.  How are you? Fine; thanks: well... And 3.5 is a number\nlast")
    assert got == [("Hello there.", "."), ("How are you?", "."), ("Fine;", ";"), ("thanks:", ";"), ("well...", "."),
                   ("And 3.5 is a number\nlast", ".")]
    assert split_sentences("") == [] and split_sentences("  \n ") == []
    assert set(c for _, c in got) <= set(PAUSES_MS)


def test_split_sentences_drops_pieces_without_a_phone():
    assert split_sentences("... !!! One. ?! -- ; Two") == [("One.", "."), ("Two", ".")]
    assert split_sentences("?!") == []


def test_split_sentences_over_long_pieces():
    text = "alpha beta, gamma delta epsilon zeta eta theta, iota kappa lambda mu nu xi omicron pi rho sigma tau."
    got = split_sentences(text, max_chars=30)
    assert all(len(s) <= 30 for s, _ in got), got
    assert got[0] == ("alpha beta,", ",")                                          # the last comma before the limit
    assert got[-1][1] == "." and got[-1][0].endswith("tau.")
    assert [c for _, c in got].count(" ") >= 1                                     # no comma within the limit: the last blank
    nospace = split_sentences("x" * 75, max_chars=30)                              # neither: cut at the limit
    assert [len(s) for s, _ in nospace] == [30, 30, 15] and [c for _, c in nospace] == [" ", " ", "."]
    for t, m in ((text, 30), (text, 200), ("Hello there.  How are you? Fine; thanks: ok.", 200), ("x" * 75, 30)):
        assert "".join(s for s, _ in split_sentences(t, m)).replace(" ", "") == "".join(t.split())   # only white space is lost
    with pytest.raises(ValueError):
        split_sentences("a", max_chars=0)


def test_header_and_binding_agree_on_the_join_entry_points():
    hdr = open(os.path.join(ROOT, "include", "zvx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(zvx_[a-z0-9_]+)\s*\(", code))
    for name in ("zvx_trim_bounds", "zvx_join"):
        assert name in declared and name in _lib.EXPORTS, name
    assert re.search(r"\bZVX_T_JOIN\s*=\s*7\b", code) and re.search(r"\bZVX_T_COUNT\s*=\s*8\b", code)
    assert _lib.ZVX_T_JOIN == 7 and _lib.ZVX_T_COUNT == 8
    m = re.search(r"typedef struct zvx_join_params \{(.*?)\} zvx_join_params;", code, flags=re.S)
    assert m, "zvx_join_params not declared"
    fields = []
    for decl in m.group(1).split(";"):
        toks = decl.replace(",", " ").split()
        if toks:
            fields += [(name, toks[0]) for name in toks[1:]]
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for n, t in fields] == list(_lib.JoinParams._fields_), fields
    assert C.sizeof(_lib.JoinParams) == sum(C.sizeof(t) for _, t in _lib.JoinParams._fields_) == 20


def test_library_exports_the_join_entry_points():
    lib = _lib.load()
    for name in ("zvx_trim_bounds", "zvx_join"):
        assert getattr(lib, name) is not None
