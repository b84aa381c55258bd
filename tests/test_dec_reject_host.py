"""The decoder's entry points reject exactly as tests/golden/dec_reject_matrix.json records: the same return code,
the same text (entry-point prefix included) and, where a call has two defects, the same one reported.  The cases
are those of tests/dec_reject_cases.py; each is rejected before any launch, so this runs without a GPU."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_reject_cases as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dec_reject_matrix.json")


def test_every_decoder_entry_point_rejects_as_recorded(stif):
    L = stif._lib
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(want["entries"]) == set(R.ENTRIES)
    # every recorded case is a rejection: nothing below can reach a launch with the fake pointers
    assert want["messages"] and all(rc == L.E_INVALID and text for rc, text in want["messages"])
    for key in R.ENTRIES:       # the same cases as recorded, none missing and none new
        assert [" + ".join(n) for n, _ in R.cases(key)] == list(want["entries"][key]), key
        assert len(want["entries"][key]) > len(R.defects_of(key)) > 8, key
    got = R.record(L, expect=want)
    for key in R.ENTRIES:
        for name, i in want["entries"][key].items():
            assert got["messages"][got["entries"][key][name]] == want["messages"][i], (key, name)
