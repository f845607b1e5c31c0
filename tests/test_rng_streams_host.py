"""The table of RNG streams (MYO_RNG_STREAMS in csrc/myo_common.h), read from the header's text: the two keys myosuite_mjx_amd/objects.py
repeats for its host twin of the object-parameter draws are the table's, no two streams share a (salt, id) pair (the header's own
static_assert, restated), and outside the table and u01 no 64-bit constant is left in csrc/."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "myosuite_mjx_amd", "csrc")


def _text(name):
    src = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _streams():
    """{name: (salt, id, stride, offset)} of the table; a counter id stays the macro's name."""
    rows = re.findall(r'^\s*X\((RS_\w+),\s*(\w+),\s*(\w+),\s*(\d+),\s*(\d+),\s*"[^"]*"\)', _text("myo_common.h"), flags=re.M)
    num = lambda t: int(t.rstrip("ul"), 0)
    return {n: (num(salt), i if i.startswith("RNG_ID_") else num(i), int(stride), int(offset)) for n, salt, i, stride, offset in rows}


def test_objects_py_repeats_the_tables_keys():
    from myosuite_mjx_amd import objects
    streams = _streams()
    assert len(streams) >= 16 and streams["RS_OBJECT"] == (objects._DRAW_KEY, 12, 1024, 0)
    mul = re.search(r"#define RNG_EPISODE_MUL (0x[0-9A-Fa-f]+)ull", _text("myo_common.h")).group(1)
    assert int(mul, 16) == objects._EPISODE_KEY


def test_streams_are_distinct_and_the_only_keys():
    streams = _streams()
    pairs = [(salt, i) for salt, i, _, _ in streams.values()]
    assert len(set(pairs)) == len(pairs)
    assert [streams[n][1] for n in list(streams)[:14]] == [1, 2, 3, 4, 5, 6, 7, 7, 8, 8, 9, 10, 11, 12]      # the ids of a reset, as they were
    for f in sorted(os.listdir(CSRC)):
        text = _text(f)
        if f == "myo_common.h":                       # the table, the episode multiplier and u01's own body
            a, b = text.index("inline float u01("), text.index("enum RngStream")
            text = text[:a] + text[b:]
        assert not re.findall(r"0x[0-9A-Fa-f]{9,}", text), f
