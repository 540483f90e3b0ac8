#!/usr/bin/env python3
"""Records what a caller is told when a host entry point refuses its arguments:   python tests/golden/make_host_messages.py

tests/golden/host_messages.json: [[entry point, case, return code, bpp_last_error()], ...] of the calls listed in
tests/host_message_cases.py, made on the product source compiled for the host emulator (tests/emu).  Recorded from the commit
BEFORE the host side moved onto one error vocabulary (ArgCheck / launched for the whole library); tests/test_host_messages.py
replays the calls and compares code and text exactly, so rerun this only where a message is meant to change."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "emu"))

import emu_binding  # noqa: E402
import host_message_cases  # noqa: E402


def main():
    rows = host_message_cases.collect(emu_binding.load())
    assert len({(r[0], r[1]) for r in rows}) == len(rows), "case names must be unique per entry point"
    with open(os.path.join(HERE, "host_messages.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d refusals of %d entry points" % (len(rows), len({r[0] for r in rows})))


if __name__ == "__main__":
    main()
