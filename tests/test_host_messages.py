"""What a caller is told when a host entry point refuses its arguments -- return code and bpp_last_error() text -- is
part of the library's behaviour: the calls of tests/host_message_cases.py, replayed on the emulated product, against the
recording tests/golden/host_messages.json (tests/golden/make_host_messages.py)."""
import json
import os

from conftest import GOLDEN

import host_message_cases


def test_refusals_keep_their_code_and_their_words(emu):
    with open(os.path.join(GOLDEN, "host_messages.json")) as f:
        want = json.load(f)
    got = host_message_cases.collect(emu)
    assert [r[:2] for r in got] == [r[:2] for r in want], "the recording and the case list have drifted apart"
    for g, w in zip(got, want):
        assert g == w
