# coding: utf-8
"""The DV3_* environment switches of the package against their table in INTEGRATION.md ("Environment switches of the
Python layer"): every variable the code reads is documented there, every documented variable is read somewhere, and
every read goes through the helpers of _lib.py (one spelling, read once)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deepvoice3_pytorch_amd")

_HELPER = re.compile(r"""_env_(?:flag|int|str)\(\s*["'](DV3_[A-Z0-9_]+)["']""")
_DIRECT = re.compile(r"""environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]\s*["'](DV3_[A-Z0-9_]+)["']""")


def _sources():
    return {p: open(p).read() for p in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))}


def _table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 2b\. Environment switches of the Python layer\n(.*?)^## ", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md lost its section of environment switches"
    rows = re.findall(r"^\| `(DV3_[A-Z0-9_]+)` \|(.*)\|\s*$", m.group(1), flags=re.M)
    assert rows, "the section holds no table rows"
    return rows


def test_every_switch_the_package_reads_is_in_the_table_and_the_other_way_round():
    read = {}
    for path, src in _sources().items():
        for name in _HELPER.findall(src) + _DIRECT.findall(src):
            read.setdefault(name, []).append(os.path.relpath(path, ROOT))
    assert read, "found no switch at all: the patterns of this test no longer match the helpers"
    documented = [name for name, _ in _table()]
    assert len(documented) == len(set(documented)), "a variable has two rows"
    undocumented = sorted(set(read) - set(documented))
    assert not undocumented, "read by the package, missing from INTEGRATION.md: %s" % {n: read[n] for n in undocumented}
    stale = sorted(set(documented) - set(read))
    assert not stale, "in the table of INTEGRATION.md, read nowhere in the package: %s" % stale


def test_every_row_gives_default_place_meaning_and_measurement():
    for name, rest in _table():
        cells = [c.strip() for c in rest.split("|")]
        assert len(cells) == 4 and all(cells), (name, cells)


def test_switches_are_read_through_the_helpers_only_and_once():
    seen = {}
    for path, src in _sources().items():
        rel = os.path.relpath(path, ROOT)
        assert not _DIRECT.findall(src), "%s reads a DV3_* variable from os.environ itself: use _lib._env_*" % rel
        for name in _HELPER.findall(src):
            seen.setdefault(name, []).append(rel)
    twice = {n: w for n, w in seen.items() if len(w) > 1}
    assert not twice, "read in more than one place: %s" % twice
