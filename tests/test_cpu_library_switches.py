# coding: utf-8
"""The library's run-time switches: the DV3_SWITCHES list of include/dv3hip.h (read as _lib.SWITCHES, no library load)
against its table in INTEGRATION.md ("Run-time switches of the library"), in both directions, id and default included;
no id twice, no retired id back in the list; and the tests name switches by DV3_SW_* -- a numeric first argument of
dv3_debug_set belongs to the refusal test alone."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepvoice3_pytorch_amd import _lib  # noqa: E402

# ids the library once took and refuses now ("Retired ids"): never reused
RETIRED = (1, 5, 6, 7, 8, 9, 13, 16, 21, 23, 24, 25, 26, 27, 28, 32, 42, 43, 45, 46)
REFUSAL_TEST = ("test_gpu_kernels.py", "test_debug_set_refuses_retired_and_unknown_switches")


def _section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^### Run-time switches of the library\n(.*?)^ABI 50:", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md lost its section of library switches"
    return m.group(1)


def _table():
    rows = re.findall(r"^\| `(\d+)` \| `(\w+)` \| `(-?\d+)` \|(.*)\|\s*$", _section(), flags=re.M)
    assert rows, "the section holds no table rows"
    return rows


def test_the_table_and_the_header_list_agree_in_both_directions():
    documented = {"DV3_SW_" + name: (int(i), int(d)) for i, name, d, _ in _table()}
    assert len(documented) == len(_table()), "a switch has two rows"
    assert _lib.SWITCHES, "the header's list was not parsed"
    assert documented == {name: (row[0], row[1]) for name, row in _lib.SWITCHES.items()}


def test_every_row_gives_forms_reader_and_measurement():
    for i, name, d, rest in _table():
        cells = [c.strip() for c in rest.split("|")]
        assert len(cells) == 3 and all(cells), (name, cells)


def test_ids_are_unique_in_range_and_not_retired():
    ids = [row[0] for row in _lib.SWITCHES.values()]
    assert len(ids) == len(set(ids)), "an id appears twice"
    assert not set(ids) & set(RETIRED), "a retired id is back in the list"
    assert _lib.CONSTS["DV3_DEBUG_CENSUS"] not in ids           # the census: dv3_debug_set's one special case
    for name, (i, dflt, lo, hi) in _lib.SWITCHES.items():
        assert lo <= dflt <= hi, name
        assert _lib.CONSTS[name] == i                             # the header's enum, as parse_header gives it
    listed = sorted(int(v) for part in re.findall(r"^- (.*?):", _section(), flags=re.M) for v in re.findall(r"`(\d+)`", part))
    assert listed == sorted(RETIRED), "the retired ids of INTEGRATION.md and of this test differ"


def test_tests_name_switches_not_numbers():
    call = re.compile(r"""dv3_debug_set(?:\(|["'],)\s*(\d+)\s*,""")
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        src = open(path).read()
        if os.path.basename(path) == REFUSAL_TEST[0]:     # the refusal test may: unknown and retired ids have no name
            m = re.search(r"^def %s\(.*?(?=^def )" % REFUSAL_TEST[1], src, flags=re.S | re.M)
            assert m, "the refusal test is gone"
            src = src.replace(m.group(0), "")
        found = call.findall(src)
        assert not found, "%s calls dv3_debug_set with the switch number(s) %s: use _lib.switches and DV3_SW_*" % (
            os.path.basename(path), found)
