"""Writes parse_mutants.json: the byte mutants the GPU rejection and accepted-mutant tests upload,
with what the host emitter says about each.  Data only: the generator parameters of the base
streams, then per mutant [stream index, byte position, byte value, host status, host message
detail, rejected by the scan].

The walk is tests/parse_mutants.py's: the sequences whose first 900 mutants per stream
tests/test_device_parse_cpu.py runs in full, followed here to 1500 per stream (see there).  Kept,
in sequence order: the first PER_REASON mutants per slice-level reason that the scan lets through,
and the first N_ACCEPTED mutants the host emitter accepts with records that differ from the
unmutated stream's.  tests/test_parse_mutants_cpu.py replays every entry against the live library,
so a stale file fails there.

    python tests/golden/make_parse_mutants.py        # rewrites tests/golden/parse_mutants.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import parse_mutants as PM  # noqa: E402

PER_REASON = 3
N_ACCEPTED = 24


def make():
    rejected = {r: [] for r in PM.SLICE_REASONS}
    accepted = []
    for si, (es, w, h, cf) in enumerate(PM.base_streams()):
        base = PM.host(es, w, h, cf)[2]
        for pos, val in PM.walk(si, es, PM.FIXTURE_MUTANTS_PER_STREAM):
            b = PM.mutate(es, pos, val)
            hs, hm, p = PM.host(b, w, h, cf)
            if hs == 0:
                if len(accepted) < N_ACCEPTED and not PM.same_records(base, (p.mbs, p.coefs)):
                    accepted.append([si, pos, val, 0, "", False])
                continue
            by_scan = PM.twin(b, w, h, cf)[3]
            if by_scan:
                continue
            for r in PM.SLICE_REASONS:
                if r in hm and len(rejected[r]) < PER_REASON:
                    rejected[r].append([si, pos, val, hs, PM.detail(hm), False])
    es, w, h, cf = PM.vlc0_stream()
    hs, hm, _ = PM.host(es, w, h, cf)
    return {
        "streams": PM.STREAMS,
        "walk_seed": PM.WALK_SEED,
        "mutants_per_stream": PM.FIXTURE_MUTANTS_PER_STREAM,
        "rejected": rejected,
        "accepted": accepted,
        "intra_vlc_format0": {"stream": PM.VLC0_STREAM, "status": hs, "detail": PM.detail(hm)},
    }


def dumps(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(PM.FIXTURE, "w") as f:
        f.write(dumps(make()))
    print(PM.FIXTURE)
