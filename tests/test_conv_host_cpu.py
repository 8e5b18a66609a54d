"""No GPU: the host layer (mcav.nn's conv section, mcav.tape.deconv, the networks' forward / backward engines) asks the library for exactly
the launches, in the order and with the descriptors, that the commit before its rework asked for.

tests/conv_host_log.py stands in for the library (planner entries answered by the real one, every launch recorded), tests/conv_host_cases.py
drives the public functions as the networks do, and tests/golden/conv_host_parent.json holds the sha256 of every case's log as that commit
wrote it (tests/golden/make_conv_host_golden.py; its --dump prints a case's log for a diff between two checkouts).

The one figure that may differ is a profile record's `executed` where the earlier code guessed against its own planner: those records are
listed in conv_host_cases.EXECUTED_CORRECTED, everything else of their cases is still compared, and `executed` must be what the planned
route gives."""
import json
import os

import pytest

import conv_host_cases as C
from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "conv_host_parent.json")
CHUNKS = 16


@pytest.fixture(scope="module")
def recorded():
    from mcav import lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libmcav_depth.so is not built (%s): the planner entries answer the host layer's questions" % L.LIB_PATH)
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_names_every_case(recorded):
    assert recorded["commit"] == "55fd216"
    assert list(recorded["cases"]) == sorted(C.all_cases()), "the cases changed: record the golden again at the parent commit"
    assert all((name in recorded["cases"]) for name, _ in C.EXECUTED_CORRECTED)


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_host_layer_reproduces_the_recorded_log(recorded, chunk):
    names = sorted(C.all_cases())[chunk::CHUNKS]
    got = C.hashes(names)
    bad = [n for n in names if got[n] != recorded["cases"][n]]
    assert not bad, "%d of %d cases differ from the log recorded at %s, first: %r (diff `make_conv_host_golden.py --dump` of the two checkouts)" % (
        len(bad), len(names), recorded["commit"], bad[0])


def test_corrected_records_follow_the_planned_route(recorded):
    """Each listed record: the figure the earlier code gave is the one the table says, the route is the one the table says, and the host
    layer now reports what that route executes."""
    cases = C.all_cases()
    for case in sorted({name for name, _ in C.EXECUTED_CORRECTED}):
        (log, planned) = C.run(cases[case], routes=True)[1]
        timed = [r for kind, r in planned]
        for (name, i), (parent, family, variant, value) in C.EXECUTED_CORRECTED.items():
            if name != case:
                continue
            rec, _ = log.profile[i]
            assert rec.i1 == rec.i0 + 1
            route = timed[rec.i0]
            assert (route.family, route.variant) == (family, variant), (name, i)
            assert parent != value and float(rec.executed).hex() == value, (name, i, float(rec.executed).hex())
