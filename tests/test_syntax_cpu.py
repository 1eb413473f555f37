"""CPU: the slice and macroblock syntax of the host emitter (csrc/parse.cpp) and of the CPU twin of
the device parse (csrc/slice_parse.h) against the directed streams of tests/directed_syntax.py,
an independent writer and slice-state model: the records equal the model's expected records, the
frames the oracle decodes from them have the MD5s of the compiled reference
(tests/golden/syntax/manifest.json), the streams together hold every syntax event of
directed_syntax.REQUIRED_EVENTS, and the out-of-contract streams are rejected alike."""
import json
import os

import numpy as np
import pytest

import directed_syntax as DS
import parse_mutants as PM
from conftest import GOLDEN
from helpers import oracle_frames, yuv_md5

SYNTAX = os.path.join(GOLDEN, "syntax")
with open(os.path.join(SYNTAX, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
BY_NAME = {e["name"]: e for e in MANIFEST}
POSITIVE = [e for e in MANIFEST if e["md5"] is not None]
FIELDS = ("x", "y", "flags", "cbp", "qscale", "ncoef", "coef_off", "mv")


@pytest.fixture(scope="module")
def streams():
    """every directed stream, written once: {name: Stream}"""
    return {S.name: S for S in DS.build_all()}


def read(e):
    with open(os.path.join(SYNTAX, e["file"]), "rb") as f:
        return f.read()


def test_hand_written_codes_are_the_ones_test_vlc_states():
    """macroblock_escape, the two end-of-block codes and the coefficient escape are not in the
    table fixture; tests/test_vlc.py::test_escape_eob_and_invalid_codes states the same bits"""
    assert DS.MB_ESCAPE == "00000001000"
    assert DS.EOB == {0: "10", 1: "0110"}
    assert DS.COEF_ESCAPE == "000001"
    assert len(DS.MBA) == 33 and len(DS.CBP) == 64 and len(DS.MOTION) == 33
    assert [len(DS.MBTYPE[p]) for p in (1, 2, 3)] == [2, 7, 11]
    assert len(DS.COEF[0]) == len(DS.COEF[1]) == 111 and all(len(t) == 12 for t in DS.DCSIZE)


def test_fixture_is_what_the_writer_writes(streams):
    assert sorted(streams) == sorted(e["name"] for e in POSITIVE)
    for e in POSITIVE:
        S = streams[e["name"]]
        assert read(e) == S.es, e["name"]
        assert (e["width"], e["height"], e["chroma_format"], e["frames"]) == (S.width, S.height, S.cf, S.npics)
        assert e["events"] == sorted(S.events)
    for build, status, reason in DS.NEGATIVE:
        S = build()
        e = BY_NAME[S.name]
        assert read(e) == S.es and (e["status"], e["reason"]) == (status, reason)
    # the streams at the geometry limits: under 400 KB each and 1 MB together; all others 256 KB together
    limit = {n + ".m2v": os.path.getsize(os.path.join(SYNTAX, n + ".m2v")) for n in DS.LIMIT_NAMES}
    assert max(limit.values()) < 400 * 1024 and sum(limit.values()) < 1024 * 1024
    total = sum(os.path.getsize(os.path.join(SYNTAX, n)) for n in os.listdir(SYNTAX) if n not in limit)
    assert total < 256 * 1024


@pytest.mark.parametrize("entry", POSITIVE, ids=[e["name"] for e in POSITIVE])
def test_records_equal_the_model_and_frames_equal_the_reference(streams, entry):
    S = streams[entry["name"]]
    want_mbs, want_coefs = DS.records(S)
    hs, hm, p = PM.host(S.es, S.width, S.height, S.cf)
    assert hs == 0, hm
    assert len(p.mbs) == len(want_mbs)
    for f in FIELDS:  # field by field, so that a failure names the field and the macroblock
        bad = np.nonzero((p.mbs[f] != want_mbs[f]).reshape(len(want_mbs), -1).any(1))[0]
        assert not len(bad), (f, [(int(want_mbs["y"][i]), int(want_mbs["x"][i]), i // (S.mbw * S.mbh),
                                   p.mbs[f][i].tolist(), want_mbs[f][i].tolist()) for i in bad[:3]])
    assert np.array_equal(p.coefs, want_coefs)
    ts, tm, rec, _ = PM.twin(S.es, S.width, S.height, S.cf)
    assert ts == 0, tm
    assert rec[0].tobytes() == want_mbs.tobytes() and rec[1].tobytes() == want_coefs.tobytes()
    frames = oracle_frames(p)
    assert [yuv_md5(frames[d]) for d in p.display] == entry["md5"]


def test_every_syntax_event_is_exercised(streams):
    got = set().union(*(S.events for S in streams.values()))
    want = set(DS.REQUIRED_EVENTS)
    assert len(want) == len(DS.REQUIRED_EVENTS)
    assert not want - got, sorted(want - got)
    assert got == want
    assert set().union(*(set(e["events"]) for e in POSITIVE)) == want  # and so says the committed fixture


@pytest.mark.parametrize("case", DS.NEGATIVE, ids=[c[0].__name__ for c in DS.NEGATIVE])
def test_out_of_contract_streams_are_rejected_alike(case):
    build, status, reason = case
    S = build()
    hs, hm, _ = PM.host(S.es, S.width, S.height, S.cf)
    ts, tm, _, _ = PM.twin(S.es, S.width, S.height, S.cf)
    assert hs == status and reason in hm, hm
    assert ts == status and PM.detail(tm) == PM.detail(hm), (tm, hm)
